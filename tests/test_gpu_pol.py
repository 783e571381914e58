"""GPU tests of the polarimetric EHT losses: libbhnerf_pol.so (csrc/eht_pol.hip) behind observation.PolDFT, engine.chi2_eht and
TrainStep.eht_pol -- against the float64 reference of tests/pol_cases.py, bitwise against libbhnerf_eht.so where the two compute
the same thing (the visibilities), and held to the caller-owned-buffer contract of include/bhnerf_pol.h.

Bounds (pol_cases.bound).  'pvis' is linear in the visibilities like 'vis': the project's f32 bound, 2e-5 -- the loss relative,
dimages relative to its largest element.  'm' divides by I; it and every total or gradient that contains it are NOT assumed to
meet that bound: their error against the float64 reference was measured on an MI355X (pol_cases.MEASURED_M) and the
tests bound it at ten times the measurement and never above 1e-3 -- the rule of DESIGN 4.15 for 'logcamp'.  Every case has its
smallest |I| >= 0.05 of the largest (asserted in pol_cases.case)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
import pol_cases as P                                                  # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401

ARRAYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eht_arrays')


def _chi2(c, dtype, dev, want_grad=True, scale=1.0, weights=None, op=None, images=None, data=None):
    """engine.chi2_eht on the PolDFT of a case -> (loss[1], dimages, the three floats of op.last_terms as float32 NumPy)."""
    from bhnerf_amd import engine
    op = op if op is not None else P.operator(c, weights)
    target, sigma = data if data is not None else P.packed(c, dtype)
    images = torch.as_tensor(c['images'] if images is None else images, device=dev)
    loss, dimg = engine.chi2_eht(images, op, target, sigma, scale, dtype, want_grad=want_grad)
    assert loss.shape == (1,) and op.last_terms.shape == (3,) and op.last_terms.dtype == torch.float32
    return loss, dimg, op.last_terms.cpu().numpy()


@pytest.mark.parametrize('name,Sx', P.PARAMS)
def test_parity_with_float64(dev, name, Sx):
    """Measured on an MI355X over pol_cases.PARAMS, weights {pvis: 0.5, m: 0.25}, scale 2, with and without gradient -- the largest
    relative errors against the float64 reference: 'm' and the totals that hold it 1.3e-7 (loss: the 'pvis+m' total at 13x7, Sx 4;
    the 'm' term itself 8.6e-8), 3.8e-7 (dimages, relative to the largest element: 'pvis+m' at 8x8, Sx 4): pol_cases.MEASURED_M,
    bounded at ten times that, 1.3e-6 / 3.8e-6.  'pvis' alone: 1.2e-7 / 3.1e-7 against its bound of 2e-5."""
    c = P.case(name, Sx)
    for want_grad in (True, False):
        for dtype in P.DTYPES:
            terms = dtype.split('+')
            ref = P.reference(c, dtype, P.WEIGHTS, P.SCALE)
            loss, dimg, three = _chi2(c, dtype, dev, want_grad, P.SCALE, P.WEIGHTS)
            assert loss.item() == three[0] and all(three[1 + P.TERMS.index(t)] == 0 for t in P.TERMS if t not in terms)
            assert three[0] == np.float32(three[1] + three[2])
            parts = {t: float(three[1 + P.TERMS.index(t)]) for t in terms}
            if want_grad:
                assert dimg.shape == c['images'].shape and dimg.dtype == torch.float32
                assert Sx == 3 or not bool(dimg[:, 3].any())                               # the V plane: zeros
            else:
                assert dimg is None
            err = P.errors(dtype, loss.item(), parts, dimg.cpu().numpy() if want_grad else None, ref)
            print('\n[pol] %s Sx %d %-7s %s' % (name, Sx, dtype, '  '.join('%s %.1e' % kv for kv in err.items())), end='')
            for t in terms:
                assert err[t] <= P.bound([t], 'loss'), (dtype, t, err)
            assert err['total'] <= P.bound(terms, 'loss'), (dtype, err)
            if want_grad:
                assert err['dimages'] <= P.bound(terms, 'dimages'), (dtype, err)
    print()


def _raw(c, dev):
    """The library called directly on a case: call(terms, loss, dimages, ws, ws_bytes, Sx=, N=) -> rc, and what it holds."""
    from bhnerf_amd import _hip
    lib = _hip.pol_lib()
    H, W, B, Sx = c['H'], c['W'], c['B'], c['Sx']
    N, nvis = B * Sx, len(c['pairs'])
    img = torch.as_tensor(c['images'], device=dev).contiguous()
    uv = torch.as_tensor(c['uv'], device=dev)
    held = {t: [torch.as_tensor(a, device=dev).contiguous() for a in c['data'][t]] for t in P.TERMS}
    structs = {t: _hip.bhn_pol_term(v[0].data_ptr(), v[1].data_ptr(), 1.0) for t, v in held.items()}
    need = int(lib.bhn_pol_ws_bytes(N, nvis, H, W))
    assert need > 0

    def call(terms, loss, dimages, ws, ws_bytes, Sx=Sx, N=N):
        ref_of = lambda t: C.byref(structs[t]) if t in terms else None
        return lib.bhn_pol_chi2(_hip.ptr(img), _hip.ptr(uv), N, Sx, nvis, H, W, E.FOV / W, E.FOV / H, ref_of('pvis'), ref_of('m'), 1.0, loss, dimages,
                                ws, ws_bytes, _hip.stream_ptr(dev))
    return dict(call=call, need=need, N=N, nvis=nvis, keep=(img, uv, held, structs))


@pytest.mark.parametrize('name,Sx', [('13x7', 3), ('12x20', 4), ('8x8', 3)])
def test_workspace_visibilities_are_the_uv_librarys_bit_for_bit(dev, name, Sx):
    """The reference here is libbhnerf_eht.so (bhn_eht_vis), not the new code: V sits in the workspace where the (u, v) library's
    plan puts it."""
    from bhnerf_amd import _hip, engine, observation
    c = P.case(name, Sx)
    r = _raw(c, dev)
    N, nvis = r['N'], r['nvis']
    ws = torch.full((r['need'],), 0xFF, dtype=torch.uint8, device=dev)
    loss = torch.empty((3,), dtype=torch.float32, device=dev)
    assert r['call'](P.TERMS, _hip.ptr(loss), None, _hip.ptr(ws), r['need']) == 0
    torch.cuda.synchronize()
    a256 = lambda v: (v + 255) // 256 * 256
    eht_bytes = int(_hip.eht_lib().bhn_eht_ws_bytes(N, nvis, 0, c['H'], c['W']))
    off_vis = eht_bytes - a256(4 * N) - a256(8 * N * nvis)                              # EhtPlan: ..., V, dphi (none), loss slots
    got = ws[off_vis:off_vis + 8 * N * nvis].view(torch.float32).reshape(c['B'], Sx, nvis, 2)
    want = engine.eht_vis_uv(torch.as_tensor(c['images'], device=dev), observation.DirectDFT(c['uv'], E.FOV, (c['H'], c['W'])).to(dev))
    assert torch.equal(got, torch.view_as_real(want))
    assert E.rel_max(want.cpu().numpy(), c['vis']) <= E.F32_TOL
    assert torch.equal(torch.view_as_real(P.operator(c).observe(c['images'])), torch.view_as_real(want))       # PolDFT.observe is DirectDFT's


def test_bitwise_reproducible_and_independent_of_the_batch(dev):
    c = P.case('12x20', 3)
    for dtype in P.DTYPES:
        op = P.operator(c, P.WEIGHTS)
        loss, dimg, three = _chi2(c, dtype, dev, op=op)
        loss2, dimg2, three2 = _chi2(c, dtype, dev, op=op)
        assert torch.equal(loss, loss2) and torch.equal(dimg, dimg2) and three.tobytes() == three2.tobytes()
        assert _chi2(c, dtype, dev, want_grad=False, op=op)[2].tobytes() == three.tobytes()                     # forward only: the same floats
        # every frame alone (B = 1) is its row of the B = 3 call, bit for bit; B = 3 adds the frames' terms in the one fixed order
        # of eht_terms_sum_kernel<2> (three lanes of one wave: the xor butterfly pairs lane 0 with lane 2 first, then with lane 1)
        tgt, sig = P.packed(c, dtype)
        alone = []
        for b in range(3):
            _, dimg1, three1 = _chi2(c, dtype, dev, op=op.take([b]), images=c['images'][b:b + 1], data=(tgt[b:b + 1], sig[b:b + 1]))
            assert torch.equal(dimg1[0], dimg[b]), b
            alone.append(three1[1:])
        alone = np.array(alone, dtype=np.float32)
        assert ((alone[0] + alone[2]) + alone[1]).astype(np.float32).tobytes() == three[1:].tobytes()
        # scale 2, weight 1 and scale 1, weight 2: one effective scale, the same bits
        la, da, fa = _chi2(c, dtype, dev, scale=2.0)
        lb, db, fb = _chi2(c, dtype, dev, scale=1.0, weights={t: 2.0 for t in dtype.split('+')})
        assert torch.equal(la, lb) and torch.equal(da, db) and fa.tobytes() == fb.tobytes()
    # a term alone at weight 1 is its value in the combined call; the combined gradient is the sum of the two at the bound
    lb, db, both = _chi2(c, 'pvis+m', dev)
    lp, dp, pv = _chi2(c, 'pvis', dev)
    lm, dm, mm = _chi2(c, 'm', dev)
    assert pv[1] == both[1] == pv[0] and mm[2] == both[2] == mm[0] and pv[2] == 0 and mm[1] == 0
    want = dp.double() + dm.double()
    assert float((db.double() - want).abs().max() / want.abs().max()) <= P.bound(['m'], 'dimages')


GUARD = 4096          # bytes on either side of a buffer: 0xA5 there, the buffer itself poisoned with NaN bytes (0xFF)


@pytest.mark.parametrize('dtype', P.DTYPES)
@pytest.mark.parametrize('name,Sx', [('13x7', 4), ('12x20', 3), ('8x8', 4)])
def test_buffer_contract(dev, name, Sx, dtype):
    from bhnerf_amd import _hip
    c = P.case(name, Sx)
    r = _raw(c, dev)
    terms = dtype.split('+')
    N, nvis, need, call = r['N'], r['nvis'], r['need'], r['call']
    npix = N * c['H'] * c['W']
    mk = lambda label, nbytes: Guarded(label, nbytes, 0xFF, dev, guard=GUARD, guard_fill=0xA5)
    loss, dimg, ws = mk('loss', 12), mk('dimages', 4 * npix), mk('ws', need)
    intact = lambda *bufs: all(b.disturbed() is None for b in bufs)
    # one byte too little workspace, two Stokes planes, no term: refused, nothing launched
    assert call(terms, loss.ptr, dimg.ptr, ws.ptr, need - 1) == _hip.BHN_EWORKSPACE
    with pytest.raises(_hip.HipError, match='workspace'):
        _hip.pol_check(_hip.BHN_EWORKSPACE)
    assert call(terms, loss.ptr, dimg.ptr, ws.ptr, need, Sx=2, N=2 * c['B']) == _hip.BHN_EINVAL
    assert b'Sx must be 3 or 4' in _hip.pol_lib().bhn_pol_last_error()
    assert call((), loss.ptr, dimg.ptr, ws.ptr, need) == _hip.BHN_EINVAL
    assert b'no term present' in _hip.pol_lib().bhn_pol_last_error()
    torch.cuda.synchronize()
    assert loss.untouched() and dimg.untouched() and ws.untouched()
    # forward only: the would-be gradient buffer stays poisoned, and so does gv, the one workspace region of the backward pass
    assert call(terms, loss.ptr, None, ws.ptr, need) == 0
    torch.cuda.synchronize()
    ref_total, ref_grad, ref_parts, _ = P.reference(c, dtype)
    three = loss.f32().copy()
    assert dimg.untouched() and np.isfinite(three).all() and abs(float(three[0]) - ref_total) <= P.bound(terms, 'loss') * abs(ref_total)
    assert intact(loss, ws, dimg)
    eht_bytes = int(_hip.eht_lib().bhn_eht_ws_bytes(N, nvis, 0, c['H'], c['W']))
    assert bool((ws.mid[eht_bytes:eht_bytes + 8 * N * nvis] == 0xFF).all())
    # loss and gradient into poisoned buffers of exactly the documented sizes
    loss.mid.fill_(0xFF); ws.mid.fill_(0xFF)
    assert call(terms, loss.ptr, dimg.ptr, ws.ptr, need) == 0
    torch.cuda.synchronize()
    got = dimg.f32().reshape(ref_grad.shape)
    assert np.isfinite(got).all() and np.isfinite(loss.f32()).all()                        # every element written
    assert Sx == 3 or not got[:, 3].any()                                                  # the V plane: zeros
    assert loss.f32().tobytes() == three.tobytes()
    assert intact(loss, ws, dimg)
    assert E.rel_max(got, ref_grad) <= P.bound(terms, 'dimages')
    for t in terms:
        assert abs(float(three[1 + P.TERMS.index(t)]) - ref_parts[t]) <= P.bound([t], 'loss') * abs(ref_parts[t]), t


@pytest.mark.parametrize('name,Sx', [('12x20', 3), ('9x11', 4)])
def test_infinite_sigma_is_exactly_no_weight(dev, name, Sx):
    c = P.case(name, Sx)
    rng = np.random.default_rng(7)
    off = rng.uniform(size=c['data']['m'][1].shape) < 1.0 / 3.0
    assert off.any() and (~off).any()
    for dtype in P.DTYPES:
        terms = dtype.split('+')
        res = []
        for shift in (0.0, 3.0 - 2.0j):
            data = {t: (np.where(off, tg + np.complex64(shift), tg), np.where(off, np.float32(np.inf), sg)) for t, (tg, sg) in c['data'].items()}
            packed = P.packed(dict(c, data=data), dtype)
            res.append(_chi2(c, dtype, dev, data=packed) + (data,))
        (l0, d0, t0, data0), (l1, d1, t1, _) = res
        assert torch.equal(l0, l1) and torch.equal(d0, d1) and t0.tobytes() == t1.tobytes() and bool(torch.isfinite(d0).all())
        # the rest: the float64 reference over the finite entries (an infinite sigma is an exact zero there too)
        total, grad, parts, _ = P.pol_loss(c['images'], c['A128'], data0, terms, {t: 1.0 for t in terms}, 1.0)
        assert np.isfinite(grad).all() and 0 < total < P.reference(c, dtype)[0]
        assert abs(l0.item() - total) <= P.bound(terms, 'loss') * abs(total)
        assert E.rel_max(d0.cpu().numpy(), grad) <= P.bound(terms, 'dimages')


def test_zero_intensity_rule(dev):
    """A frame whose I plane is exactly zero: 'm' contributes 0 there and no gradient, nothing is NaN; 'pvis' does not care."""
    c = P.case('12x20', 3)
    images = c['images'].copy()
    images[0, 0] = 0.0
    full = _chi2(c, 'm', dev)
    loss, dimg, three = _chi2(c, 'm', dev, images=images)
    assert np.isfinite(three).all() and bool(torch.isfinite(dimg).all()) and not bool(dimg[0].any()) and torch.equal(dimg[1:], full[1][1:])
    assert 0 < three[2] < full[2][2]
    loss, dimg, three = _chi2(c, 'pvis+m', dev, images=images)
    assert np.isfinite(three).all() and bool(torch.isfinite(dimg).all()) and not bool(dimg[0, 0].any()) and bool(dimg[0, 1].any())
    assert three[1] == _chi2(c, 'pvis', dev)[2][1]


def _stokes_network(dev):
    """A 4x128 bf16 network on 12 x 12 rays x 24 samples with the Stokes factors of three planes, three frames, five stations."""
    from bhnerf_amd import network, synthetic, units
    H = W = 12
    geo = synthetic.synthetic_geodesics(H, W, 24, S=3, seed=2)
    t_frames = np.linspace(0, 0.5, 3)
    rng = np.random.default_rng(21)
    pos = rng.normal(size=(3, 5, 2)) * 0.5e9
    pairs = np.array([(i, j) for i in range(5) for j in range(i + 1, 5)])
    uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])
    pred = network.NeRF_Predictor(8.0, 0.0, np.inf, np.inf, net_depth=4, net_width=128, mode='bf16', device=dev)
    rt = network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'],
                                      Sigma=geo['Sigma'], t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr, J=geo['J'])
    params = pred.init_params(rt, seed=3)
    with torch.no_grad():                                  # emission sigmoid(out - 10): a large bias makes the image visible
        pred.engine().unflatten(params.flat)['MLP_0']['Dense_4']['bias'] += 6.0
    data = {'pvis': ((rng.normal(size=(3, 10)) + 1j * rng.normal(size=(3, 10))).astype(np.complex64), np.full((3, 10), 0.5, dtype=np.float32)),
            'm': ((0.3 * (rng.normal(size=(3, 10)) + 1j * rng.normal(size=(3, 10)))).astype(np.complex64), np.full((3, 10), 0.1, dtype=np.float32))}
    return dict(H=H, W=W, t_frames=t_frames * units.hr, uv=uv, pred=pred, rt=rt, params=params, data=data)


def test_one_training_step_is_the_hand_built_step(dev):
    """TrainStep.eht_pol on 12 x 12 rays x 24 samples, 4x128 bf16, three Stokes planes, B = 3: loss, gradient and parameters are
    bitwise those of render -> engine.chi2_eht_pol -> backward -> Adam written out here; network.test_eht returns the same loss
    and steps nothing; engine.chi2_eht routes a PolDFT to chi2_eht_pol."""
    from bhnerf_amd import engine, network, observation, optimization, units
    s = _stokes_network(dev)
    hp = {'num_iters': 10, 'lr_init': 1e-4, 'lr_final': 1e-5, 'seed': 3}
    weights, scale, idx = {'pvis': 0.5, 'm': 2.0}, 1.5, np.arange(3)
    for dtype in ('m', 'pvis+m'):
        terms = dtype.split('+')
        step = optimization.TrainStep.eht_pol(s['t_frames'], s['uv'], E.FOV, (s['H'], s['W']), {t: s['data'][t] for t in terms}, weights=weights,
                                              scale=scale)
        assert step.num_losses == 1 and str(step.dtype[0]) == dtype
        opt = optimization.Optimizer(hp, s['pred'], s['rt'])
        with torch.no_grad():
            opt.state.flat.copy_(s['params'].flat)
        test_loss, _, test_imgs = step(opt.state, s['rt'], idx, update_state=False)
        assert opt.state.step == 0 and torch.equal(opt.state.flat, s['params'].flat)
        loss, state, imgs = step(opt.state, s['rt'], idx)
        assert imgs.shape == (1, 3, 3, s['H'], s['W']) and state.step == 1 and float((state.flat - s['params'].flat).abs().max()) > 0
        assert float(loss.sum()) == float(test_loss.sum()) and torch.equal(imgs, test_imgs) and np.isfinite(float(loss.sum()))
        # the same step by hand
        hand = optimization.Optimizer(hp, s['pred'], s['rt'])
        with torch.no_grad():
            hand.state.flat.copy_(s['params'].flat)
        rt = s['rt']
        pred = s['pred']
        eng = pred.engine()
        geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], rt['J'], rt['g'], rt['dtau'], rt['Sigma'])
        tM0, _ = network._frame_offsets(units.strip(s['t_frames']), units.hr, rt['t_start_obs'], rt['t_injection'], eng.device)
        assert geom.Sx == 3
        eng.pack(hand.state.flat)
        taped = eng.fits_tape(3, geom.P_eff)
        images = (eng.render_train if taped else eng.render)(geom, tM0)
        op = observation.PolDFT(s['uv'], E.FOV, (s['H'], s['W']), weights=weights)
        target = np.concatenate([s['data'][t][0] for t in terms], axis=-1)
        sigma = np.concatenate([s['data'][t][1] for t in terms], axis=-1)
        hloss, dimg = engine.chi2_eht_pol(images, op, target, sigma, scale, dtype)
        rloss, rdimg = engine.chi2_eht(images, op, target, sigma, scale, dtype)
        assert torch.equal(hloss, rloss) and torch.equal(dimg, rdimg)
        n = eng.nparams
        buf = hand.state.grad_buffer()
        (eng.render_bwd_tape if taped else eng.render_bwd)(geom, tM0, dimg, out=buf[:n])
        hand.state.apply_gradients(buf[:n])
        assert float(loss.sum()) == hloss.item()
        assert torch.equal(state.grad[:n], hand.state.grad[:n]) and float(state.grad[:n].abs().max()) > 0
        assert torch.equal(state.flat, hand.state.flat)
        assert torch.equal(imgs[0].reshape(images.shape), images)
    # a render of one plane cannot feed the polarimetric terms
    with pytest.raises(AttributeError, match='3 or 4 planes'):
        engine.chi2_eht(images[:, :1].contiguous(), op, target, sigma, scale, dtype)


def test_station_gains_do_not_reach_m(dev):
    """'m' data from gained and from clean noise-free observe_same visibilities give the same loss within the bound; the 'vis'
    losses of the same two data sets differ by more than a hundred times that.  Default gains (10 % amplitudes, random phases):
    the targets of the two sets against one sigma (a gain changes a baseline's signal-to-noise ratio, so the quoted sigma of 'm'
    follows the amplitude gains; the target does not).  Phase-only gains: target and sigma of each set as Observation.data gives
    them."""
    from bhnerf_amd import constants, engine, observation, synthetic
    array = observation.Array.load_txt(os.path.join(ARRAYS, 'EHT2017.txt'))
    obs = observation.empty_eht_obs(array, 12, 60.0, timetype='GMST', times=np.linspace(19.0, 24.0, 12))
    npix = 16
    geo = synthetic.synthetic_geodesics(npix, npix, 24, seed=2)
    t_frames = np.linspace(0.0, 0.5, 12)
    planes = [synthetic.hotspot_movie(geo, t_frames, constants.GM_c3('hr'), orbit_radius=r, sigma=sg) for r, sg in ((5.5, 0.7), (4.5, 0.9), (6.0, 0.6))]
    norm = 2.0 / planes[0].sum(axis=(1, 2)).mean()
    movie = np.stack([planes[0] * norm, 0.4 * planes[1] * norm, -0.3 * planes[2] * norm], axis=1).astype(np.float32)
    clean = observation.observe_same(movie, obs, E.FOV, thermal_noise=False)
    assert clean.shape == (12, 3, obs.nvis) and clean.tobytes() == observation.observe_same(movie, obs, E.FOV, thermal_noise=False, gains=None).tobytes()
    images = torch.as_tensor(E.blobs(np.random.default_rng(5), (12, 3, npix, npix)), device=dev)
    pol, plain = obs.pol_dft(E.FOV, npix), obs.dft(E.FOV, npix)
    bound = P.bound(['m'], 'loss')
    for label, gains, own_sigma in (('default gains', observation.station_gains(obs, seed=4), False),
                                    ('phase-only gains', observation.station_gains(obs, amp_sigma=0.0, seed=4), True)):
        gained = observation.observe_same(movie, obs, E.FOV, thermal_noise=False, gains=gains)
        assert gained.tobytes() == observation.observe_host(clean, obs, False, gains=gains).tobytes()
        dc, dg = obs.data(clean, 'm', debias=False)['m'], obs.data(gained, 'm', debias=False)['m']
        assert np.isfinite(dc[1]).sum() == obs.up.sum() == np.isfinite(dg[1]).sum()
        lc = engine.chi2_eht(images, pol, dc[0], dc[1], 1.0, 'm', want_grad=False)[0].item()
        lg = engine.chi2_eht(images, pol, dg[0], dg[1] if own_sigma else dc[1], 1.0, 'm', want_grad=False)[0].item()
        vc, vg = obs.data(clean[:, 0], 'vis')['vis'], obs.data(gained[:, 0], 'vis')['vis']
        assert np.array_equal(vc[1], vg[1])
        wc = engine.chi2_eht(images[:, 0].contiguous(), plain, vc[0], vc[1], 1.0, 'vis', want_grad=False)[0].item()
        wg = engine.chi2_eht(images[:, 0].contiguous(), plain, vg[0], vg[1], 1.0, 'vis', want_grad=False)[0].item()
        print("\n[pol] %s: 'm' loss %.6e clean, %.6e gained (relative difference %.1e); 'vis' loss %.6e clean, %.6e gained (%.1e)"
              % (label, lc, lg, abs(lg - lc) / lc, wc, wg, abs(wg - wc) / wc), end='')
        assert np.isfinite([lc, lg, wc, wg]).all() and lc > 0 and wc > 0
        assert abs(lg - lc) <= bound * lc
        assert abs(wg - wc) > 100.0 * bound * wc
    print()
