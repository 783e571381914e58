"""GPU tests of the matrix-free EHT losses: libbhnerf_eht.so (csrc/eht_uv.hip) behind observation.DirectDFT, engine.chi2_eht,
loss_fn_eht and TrainStep.eht_uv, against the float64 table-form reference of tests/eht_uv_cases.py, against the dense kernels
(bhn_chi2_eht) fed DirectDFT.dense(), and held to the caller-owned-buffer contract of include/bhnerf_eht.h.

Bounds: the project's f32 bound, 2e-5 -- the loss relative, visibilities and dimages relative to their largest element.  A
'cphase' case must have its smallest visibility amplitude >= 0.05 of the largest (asserted on the float64 reference), so that
no case sits on the 1 / |vis| pole of the closure-phase gradient."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401

DTYPES = ('vis', 'amp', 'cphase')
# relative L2 between the parameter gradients of the matrix-free and the dense training step, measured on an MI355X (DESIGN
# 4.10): 'vis' 16x16 rays, 'cphase' 12x20 rays.  The tests bound it at ten times the measurement (box-to-box libm and ordering
# differences) and never above 1e-3.
MEASURED_STEP_GRAD_L2 = {'vis': 6.43e-8, 'cphase': 9.08e-7}
STEP_GRAD_BOUND = {k: min(10.0 * v, 1e-3) for k, v in MEASURED_STEP_GRAD_L2.items()}


def _chi2(c, dtype, dev, want_grad=True, scale=1.0, op=None, images=None):
    from bhnerf_amd import engine
    images = torch.as_tensor(c['images'] if images is None else images, device=dev)
    target, sigma = c['data'][dtype]
    return engine.chi2_eht(images, op if op is not None else E.operator(c, dtype), target, sigma, scale, dtype, want_grad=want_grad)


@pytest.mark.parametrize('want_grad', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,Sx', [('12x20', 0), ('13x7', 0), ('12x20', 2)])
def test_parity_with_float64_and_with_the_dense_kernels(dev, name, Sx, dtype, want_grad):
    from bhnerf_amd import engine
    c = E.case(name, Sx)
    assert c['min_amp'] >= E.MIN_AMP, c['min_amp']
    ref_loss, ref_grad, _ = c['ref'][dtype]
    op = E.operator(c, dtype)
    loss, dimg = _chi2(c, dtype, dev, want_grad, op=op)
    target, sigma = c['data'][dtype]
    flat = torch.as_tensor(c['images'], device=dev).reshape(c['images'].shape[:-2] + (-1,))
    A = op.dense()
    if Sx:                                                             # the dense path takes a matrix per Stokes plane
        A = np.stack([A] * Sx, axis=1)
    dloss, ddimg = engine.chi2_eht(flat, A, target, sigma, 1.0, dtype, want_grad=want_grad)
    e_loss, e_dense = abs(loss.item() - ref_loss) / abs(ref_loss), abs(loss.item() - dloss.item()) / abs(dloss.item())
    print('\n[eht uv] %s Sx %d %-6s loss: vs float64 %.1e, vs dense %.1e' % (name, Sx, dtype, e_loss, e_dense), end='')
    assert e_loss <= E.F32_TOL and e_dense <= E.F32_TOL, (loss.item(), ref_loss, dloss.item())
    if not want_grad:
        assert dimg is None
        return
    assert dimg.shape == c['images'].shape and dimg.dtype == torch.float32
    got = dimg.cpu().numpy()
    e_grad, e_gd = E.rel_max(got, ref_grad), E.rel_max(got, ddimg.cpu().numpy().reshape(got.shape))
    print('  dimages: vs float64 %.1e, vs dense %.1e' % (e_grad, e_gd))
    assert e_grad <= E.F32_TOL and e_gd <= E.F32_TOL, (e_grad, e_gd)


@pytest.mark.parametrize('name,Sx', [('12x20', 0), ('13x7', 0), ('12x20', 2)])
def test_observe_gives_the_float64_visibilities(dev, name, Sx):
    c = E.case(name, Sx)
    vis = E.operator(c, 'vis').observe(c['images'])
    assert vis.is_cuda and vis.dtype == torch.complex64 and tuple(vis.shape) == c['ref']['vis'][2].shape
    err = E.rel_max(vis.cpu().numpy(), c['ref']['vis'][2])
    print('\n[eht uv] observe %s Sx %d: %.1e' % (name, Sx, err))
    assert err <= E.F32_TOL
    # the operator with triangles observes the same baselines; a device-resident operator and movie are taken as they are
    op = E.operator(c, 'cphase').to(dev)
    assert torch.equal(op.observe(torch.as_tensor(c['images'], device=dev)), vis)


@pytest.mark.parametrize('dtype', ['cphase', 'vis'])
def test_a_size_the_dense_form_cannot_hold(dev, dtype):
    """20 stations: 190 baselines, 1140 triangles, every baseline in 18 of them; 64 x 64 pixels, two frames.  The dense 'cphase'
    operator would be 2 x 3 x 1140 x 4096 complex64 = 224 MB here (115 GB at 256 x 256 and 64 frames); the table form needs the
    (u, v) list."""
    c = E.case('big')
    assert len(c['pairs']) == 190 and len(c['tri']) == 1140 and (np.bincount(c['tri'].ravel()) == 18).all()
    assert c['min_amp'] >= E.MIN_AMP, c['min_amp']
    ref_loss, ref_grad, ref_vis = c['ref'][dtype]
    loss, dimg = _chi2(c, dtype, dev)
    e_loss, e_grad = abs(loss.item() - ref_loss) / abs(ref_loss), E.rel_max(dimg.cpu().numpy(), ref_grad)
    print('\n[eht uv] 20 stations %-6s loss %.1e dimages %.1e (smallest |vis| / largest %.3f)' % (dtype, e_loss, e_grad, c['min_amp']))
    assert e_loss <= E.F32_TOL and e_grad <= E.F32_TOL
    if dtype == 'vis':
        assert E.rel_max(E.operator(c, 'vis').observe(c['images']).cpu().numpy(), ref_vis) <= E.F32_TOL


@pytest.mark.parametrize('dtype', DTYPES)
def test_bitwise_reproducible_independent_of_the_batch_and_linear_in_scale(dev, dtype):
    c = E.case('12x20')
    op = E.operator(c, dtype)
    loss, dimg = _chi2(c, dtype, dev, op=op)
    loss2, dimg2 = _chi2(c, dtype, dev, op=op)
    assert torch.equal(loss, loss2) and torch.equal(dimg, dimg2)
    vis = op.observe(c['images'])
    assert torch.equal(torch.view_as_real(vis), torch.view_as_real(op.observe(c['images'])))
    # frame 1 alone (B = 1) is row 1 of the B = 3 call, bit for bit
    one = dict(c, images=c['images'][1:2], data={k: (t[1:2], s[1:2]) for k, (t, s) in c['data'].items()})
    op1 = op.take([1])
    loss1, dimg1 = _chi2(one, dtype, dev, op=op1)
    assert torch.equal(dimg1[0], dimg[1])
    assert torch.equal(torch.view_as_real(op1.observe(c['images'][1:2]))[0], torch.view_as_real(vis)[1])
    loss3, dimg3 = _chi2(c, dtype, dev, scale=2.0, op=op)
    assert abs(loss3.item() - 2 * loss.item()) <= 1e-6 * abs(loss3.item())
    assert float((dimg3 - 2 * dimg).abs().max()) <= 1e-6 * float(dimg3.abs().max())


GUARD = 4096          # bytes on either side of a buffer: 0xA5 there, the buffer itself poisoned with NaN bytes (0xFF)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,Sx', [('13x7', 0), ('12x20', 2)])
def test_buffer_contract(dev, name, Sx, dtype):
    from bhnerf_amd import _hip
    lib = _hip.eht_lib()
    c = E.case(name, Sx)
    H, W, B, S = c['H'], c['W'], c['B'], max(Sx, 1)
    N, nvis = B * S, len(c['pairs'])
    ncp = len(c['tri']) if dtype == 'cphase' else 0
    target, sigma = c['data'][dtype]
    img = torch.as_tensor(c['images'], device=dev).contiguous()
    uv = torch.as_tensor(c['uv'], device=dev)
    tgt = torch.as_tensor(np.ascontiguousarray(target).view(np.float32) if dtype == 'vis' else target, device=dev).contiguous()
    sig = torch.as_tensor(sigma, device=dev).contiguous()
    tri, sign = torch.as_tensor(c['tri'], device=dev), torch.as_tensor(c['sign'], device=dev)
    need = int(lib.bhn_eht_ws_bytes(N, nvis, ncp, H, W))
    assert need > 0
    psy, psx = E.FOV / H, E.FOV / W
    stream = _hip.stream_ptr(dev)

    def call(loss, dimages, ws, ws_bytes):
        return lib.bhn_eht_chi2_uv(_hip.ptr(img), _hip.ptr(uv), N, S, nvis, H, W, psx, psy, DTYPES.index(dtype), _hip.ptr(tgt), _hip.ptr(sig),
                                   1.0, _hip.ptr(tri) if ncp else None, _hip.ptr(sign) if ncp else None, ncp, loss, dimages, ws, ws_bytes, stream)

    mk = lambda label, nbytes: Guarded(label, nbytes, 0xFF, dev, guard=GUARD, guard_fill=0xA5)
    loss, dimg, ws = mk('loss', 4), mk('dimages', 4 * N * H * W), mk('ws', need)
    intact = lambda *bufs: all(b.disturbed() is None for b in bufs)
    # one byte too little workspace: refused, nothing launched
    assert call(loss.ptr, dimg.ptr, ws.ptr, need - 1) == _hip.BHN_EWORKSPACE
    with pytest.raises(_hip.HipError, match='workspace'):
        _hip.eht_check(_hip.BHN_EWORKSPACE)
    torch.cuda.synchronize()
    assert loss.untouched() and dimg.untouched() and ws.untouched()
    # forward only: the would-be gradient buffer stays poisoned
    assert call(loss.ptr, None, ws.ptr, need) == 0
    torch.cuda.synchronize()
    ref_loss, ref_grad, ref_vis = c['ref'][dtype]
    assert dimg.untouched() and abs(float(loss.f32()[0]) - ref_loss) <= E.F32_TOL * abs(ref_loss)
    assert intact(loss, ws, dimg)
    # loss and gradient into poisoned buffers of exactly the documented sizes
    loss.mid.fill_(0xFF); ws.mid.fill_(0xFF)
    assert call(loss.ptr, dimg.ptr, ws.ptr, need) == 0
    torch.cuda.synchronize()
    got = dimg.f32().reshape(ref_grad.shape)
    assert np.isfinite(got).all() and np.isfinite(float(loss.f32()[0]))                    # every element written
    assert intact(loss, ws, dimg)
    assert E.rel_max(got, ref_grad) <= E.F32_TOL and abs(float(loss.f32()[0]) - ref_loss) <= E.F32_TOL * abs(ref_loss)
    if dtype == 'vis':                                                                     # bhn_eht_vis, the same way
        vneed = int(lib.bhn_eht_ws_bytes(N, nvis, 0, H, W))
        vis, vws = mk('vis', 8 * N * nvis), mk('ws of bhn_eht_vis', vneed)
        args = (_hip.ptr(img), _hip.ptr(uv), N, S, nvis, H, W, psx, psy, vis.ptr, vws.ptr)
        assert lib.bhn_eht_vis(*args, vneed - 1, stream) == _hip.BHN_EWORKSPACE
        torch.cuda.synchronize()
        assert vis.untouched() and vws.untouched()
        assert lib.bhn_eht_vis(*args, vneed, stream) == 0
        torch.cuda.synchronize()
        v = vis.f32().view(np.complex64).reshape(ref_vis.shape)
        assert np.isfinite(v.view(np.float32)).all() and intact(vis, vws)
        assert E.rel_max(v, ref_vis) <= E.F32_TOL


def _network_case(H, W, dev, seed, spread=3e9):
    """A 4x64 f32 network on H x W rays x 24 samples with a visible image, three frames, and a 5-station operator with stations
    `spread` wavelengths apart."""
    from bhnerf_amd import constants, network, synthetic, units
    geo = synthetic.synthetic_geodesics(H, W, 24, seed=2)
    t_frames = np.linspace(0, 0.5, 3)
    movie = synthetic.hotspot_movie(geo, t_frames, constants.GM_c3('hr'))
    movie = movie * (2.0 / movie.sum(axis=(1, 2)).mean())
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(3, 5, 2)) * spread
    pairs = np.array([(i, j) for i in range(5) for j in range(i + 1, 5)])
    uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])
    pred = network.NeRF_Predictor(8.0, 0.0, np.inf, np.inf, net_depth=4, net_width=64, mode='f32', device=dev)
    rt = network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'],
                                      Sigma=geo['Sigma'], t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr)
    params = pred.init_params(rt, seed=3)
    with torch.no_grad():                                  # emission sigmoid(out - 10): a large bias makes the image visible
        pred.engine().unflatten(params.flat)['MLP_0']['Dense_4']['bias'] += 6.0
    vis = np.einsum('tkp,tp->tk', E.dense128(uv, E.FOV, H, W), movie.reshape(3, -1).astype(np.complex128))
    return dict(t_frames=t_frames, movie=movie, uv=uv, pairs=pairs, pred=pred, rt=rt, params=params, vis=vis)


def test_one_training_step_matches_the_dense_step(dev):
    """TrainStep.eht_uv against TrainStep.eht_arrays on dense(): 16 x 16 rays x 24 samples, 4x64 f32, B = 3, 'vis'."""
    from bhnerf_amd import observation, optimization, units
    s = _network_case(16, 16, dev, seed=11)
    target = s['vis'].astype(np.complex64)
    sigma = np.full(target.shape, 0.1 * float(np.abs(target).mean()), dtype=np.float32)
    op = observation.DirectDFT(s['uv'], E.FOV, 16)
    steps = {'uv': optimization.TrainStep.eht_uv(s['t_frames'] * units.hr, target, sigma, s['uv'], E.FOV, 16, dtype='vis'),
             'dense': optimization.TrainStep.eht_arrays(s['t_frames'] * units.hr, target, sigma, op.dense(), dtype='vis')}
    hp = {'num_iters': 10, 'lr_init': 1e-4, 'lr_final': 1e-5, 'seed': 3}
    res = {}
    for kind, reps in (('uv', 2), ('dense', 1)):
        for rep in range(reps):
            opt = optimization.Optimizer(hp, s['pred'], s['rt'])
            with torch.no_grad():
                opt.state.flat.copy_(s['params'].flat)
            loss, state, imgs = steps[kind](opt.state, s['rt'], np.arange(3))
            assert imgs.shape == (1, 3, 16, 16) and state.step == 1
            res[(kind, rep)] = (float(loss.sum()), state.grad[:state.flat.numel()].clone(), state.flat.clone())
    assert torch.equal(res[('uv', 0)][1], res[('uv', 1)][1]) and torch.equal(res[('uv', 0)][2], res[('uv', 1)][2])      # bitwise
    assert res[('uv', 0)][0] == res[('uv', 1)][0]
    lu, gu, fu = res[('uv', 0)]
    ld, gd, _ = res[('dense', 0)]
    assert float(gd.norm()) > 0 and float((fu - s['params'].flat).abs().max()) > 0
    l2 = float((gu - gd).norm() / gd.norm())
    print('\n[eht uv] training step vis 16x16: loss uv %.6e dense %.6e, parameter gradient relative L2 %.2e' % (lu, ld, l2))
    assert abs(lu - ld) <= 1e-4 * abs(ld)
    assert l2 <= STEP_GRAD_BOUND['vis'], l2


def test_loss_fn_eht_cphase_backward_matches_the_dense_form(dev):
    """The same step on 12 x 20 images, 'cphase', through loss_fn_eht + backward."""
    from bhnerf_amd import network, observation, units
    # the untrained network's image fills the field of view: a compact array (0.5e9 wavelengths) does not resolve it out, so
    # every baseline keeps an amplitude well off the 1 / |vis| pole (asserted below on the visibilities of the rendered images)
    s = _network_case(12, 20, dev, seed=12, spread=0.5e9)
    tri, sign = observation.closure_table(s['pairs'], observation.closure_triangles(5))
    target = (E.closure_phases(s['vis'], tri, sign) + 0.3).astype(np.float32)
    sigma = np.full(target.shape, 0.1, dtype=np.float32)
    op = observation.DirectDFT(s['uv'], E.FOV, (12, 20), triangles=(tri, sign))
    res = {}
    for kind, A, reps in (('uv', op, 2), ('dense', op.dense(), 1)):
        for rep in range(reps):
            flat = s['params'].flat.detach().clone().requires_grad_(True)
            tree = network.ParamTree(); tree.flat = flat
            loss, [images] = network.loss_fn_eht(tree, s['pred'].apply, target, sigma, A, s['t_frames'], *s['rt'].values(), 1.0, units.hr, 'cphase')
            loss.backward()
            res[(kind, rep)] = (loss.item(), flat.grad.detach().clone(), images.detach())
    vis = op.observe(res[('uv', 0)][2]).cpu().numpy()
    print('\n[eht uv] loss_fn_eht cphase 12x20: smallest |vis| / largest = %.3f' % (np.abs(vis).min() / np.abs(vis).max()), end='')
    assert np.abs(vis).min() >= E.MIN_AMP * np.abs(vis).max(), (np.abs(vis).min(), np.abs(vis).max())     # off the pole
    assert res[('uv', 0)][0] == res[('uv', 1)][0] and torch.equal(res[('uv', 0)][1], res[('uv', 1)][1])                # bitwise
    lu, gu, _ = res[('uv', 0)]
    ld, gd, _ = res[('dense', 0)]
    l2 = float((gu - gd).norm() / gd.norm())
    print('\n[eht uv] loss_fn_eht cphase 12x20: loss uv %.6e dense %.6e, parameter gradient relative L2 %.2e' % (lu, ld, l2))
    assert float(gd.norm()) > 0 and abs(lu - ld) <= 1e-4 * abs(ld)
    assert l2 <= STEP_GRAD_BOUND['cphase'], l2


def test_errors_fire_before_any_launch(dev):
    from bhnerf_amd import _hip, engine, observation
    c = E.case('12x20')
    img = torch.as_tensor(c['images'], device=dev)
    tv, sv = c['data']['vis']
    tc, sc = c['data']['cphase']
    plain, closed = E.operator(c, 'vis'), E.operator(c, 'cphase')
    with pytest.raises(AttributeError):
        engine.chi2_eht(img, plain, tv, sv, 1.0, 'nope')
    with pytest.raises(AttributeError):                                # triangles with 'vis'
        engine.chi2_eht(img, closed, tv, sv, 1.0, 'vis')
    with pytest.raises(AttributeError):                                # 'cphase' without triangles
        engine.chi2_eht(img, plain, tc, sc, 1.0, 'cphase')
    with pytest.raises(AttributeError):                                # visibility count
        engine.chi2_eht(img, plain, tv[:, :9], sv[:, :9], 1.0, 'vis')
    with pytest.raises(AttributeError):                                # triangle count
        engine.chi2_eht(img, closed, tc[:, :9], sc[:, :9], 1.0, 'cphase')
    with pytest.raises(AttributeError):                                # Stokes count: two planes of target, one of images
        engine.chi2_eht(img, plain, np.stack([tv, tv], 1), np.stack([sv, sv], 1), 1.0, 'vis')
    with pytest.raises(AttributeError):                                # frame count
        engine.chi2_eht(img, plain.take([0, 1]), tv, sv, 1.0, 'vis')
    with pytest.raises(AttributeError):                                # image size
        engine.chi2_eht(img[:, :, :19], plain, tv, sv, 1.0, 'vis')
    with pytest.raises(AttributeError):
        plain.observe(c['images'][:, :11])
    lib = _hip.eht_lib()
    uv = torch.as_tensor(c['uv'], device=dev)
    out = torch.empty((3, 10, 2), dtype=torch.float32, device=dev)
    ws = torch.empty((int(lib.bhn_eht_ws_bytes(3, 10, 0, 12, 20)),), dtype=torch.uint8, device=dev)
    for change in (dict(N=0), dict(Sx=2), dict(psx=0.0), dict(images=None), dict(vis_out=None)):
        a = dict(dict(images=_hip.ptr(img), uv=_hip.ptr(uv), N=3, Sx=1, nvis=10, H=12, W=20, psx=1e-11, psy=1e-11, vis_out=_hip.ptr(out),
                      ws=_hip.ptr(ws), ws_bytes=ws.numel()), **change)
        rc = lib.bhn_eht_vis(*a.values(), _hip.stream_ptr(dev))
        assert rc == _hip.BHN_EINVAL, change
        with pytest.raises(_hip.HipError, match='libbhnerf_eht'):
            _hip.eht_check(rc)
