"""CPU tests of the polarimetric EHT losses (libbhnerf_pol.so, csrc/eht_pol.hip, observation.PolDFT) and of the station gains of
the observation layer: everything about them that needs no device.

The plan and the arithmetic of the terms live in csrc/eht_pol.h on top of csrc/eht_uv.h and compile with a plain C++ compiler.
tools/eht_pol_host.cpp walks the launches of bhn_pol_chi2 one workgroup after the other; here it is built with g++ -O2 and the
sanitizers (tests/side_lib_support.py), run as a child process with its outputs and workspace in heap blocks of exactly the
documented sizes, and compared with the float64 reference of tests/pol_cases.py.  Nothing built with a sanitizer is loaded into
this Python process.

Bounds.  'pvis' is linear in the visibilities like 'vis' and is held to the project's f32 bound (eht_uv_cases.F32_TOL: the loss
relative, dimages relative to its largest element).  'm' divides by I; on the host build it and every total or gradient that
contains it are held to M_CEILING = 1e-3, the ceiling that the measured bounds of tests/pol_cases.py (M_BOUND, used on the device)
may never exceed.  The figures are printed.  The mutants of the reference must stand out by five times the device's bound."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
import pol_cases as P                                                  # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import observation                                     # noqa: E402

ARRAYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eht_arrays')
M_CEILING = 1e-3


def bound(names):
    return M_CEILING if 'm' in names else E.F32_TOL


@pytest.fixture(scope='module')
def eht2017():
    return observation.Array.load_txt(os.path.join(ARRAYS, 'EHT2017.txt'))


@pytest.fixture(scope='module')
def track(eht2017):
    """EHT2017 on Sgr A*, 12 frames from GMST 19 h to 24 h: the station set changes along it."""
    return observation.empty_eht_obs(eht2017, 12, 60.0, timetype='GMST', times=np.linspace(19.0, 24.0, 12))


def _stokes_vis(obs, seed=1):
    """Visibilities (nt, 3, nvis) of three polarised point sources: I well off zero on every baseline, Q and U of its size."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-20e-6, 20e-6, (3, 2)) / 206265.0
    phase = np.exp(-2j * np.pi * (obs.uv[..., 0:1] * xy[:, 0] + obs.uv[..., 1:2] * xy[:, 1]))
    flux = np.array([[1.0, 0.3, 0.2], [0.3, -0.1, 0.05], [-0.2, 0.15, 0.1]])
    return np.stack([(f * phase).sum(-1) for f in flux], axis=1)


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/eht_pol_host.cpp built with the sanitizers -> run(case, dtype, ...) -> (vis, loss[3], dimages or None)."""
    exe, work = side.build_host_program(tmp_path_factory, 'eht_pol_host')

    def run(c, dtype, want_grad=True, scale=1.0, weights=None, tag='case'):
        terms = dtype.split('+')
        H, W, B, Sx = c['H'], c['W'], c['B'], c['Sx']
        N, nvis = B * Sx, len(c['pairs'])
        w = dict({t: 1.0 for t in P.TERMS}, **(weights or {}))
        present = sum(1 << P.TERMS.index(t) for t in terms)
        head = np.array([N, Sx, nvis, H, W, present, int(want_grad), E.FOV / W, E.FOV / H, scale] + [w[t] for t in P.TERMS], dtype=np.float64)
        arrays = [head, c['uv'], c['images']]
        for t in terms:
            arrays += [c['data'][t][0].astype(np.complex64), c['data'][t][1].astype(np.float32)]
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        with open(fin, 'wb') as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        npix = N * H * W
        assert len(raw) == 8 * N * nvis + 12 + (4 * npix if want_grad else 0)         # the documented sizes, nothing else
        vis = np.frombuffer(raw, dtype=np.complex64, count=N * nvis).reshape(B, Sx, nvis)
        loss = np.frombuffer(raw, dtype=np.float32, count=3, offset=8 * N * nvis)
        dimg = np.frombuffer(raw, dtype=np.float32, count=npix, offset=8 * N * nvis + 12).reshape(c['images'].shape) if want_grad else None
        return vis, loss, dimg
    return run


@pytest.mark.parametrize('name,Sx', P.PARAMS)
def test_host_build_meets_the_float64_reference(host_program, name, Sx):
    c = P.case(name, Sx)
    print('\n[pol] %s Sx %d: smallest |I| / largest = %.3f, largest |m| = %.2f' % (name, Sx, c['min_amp'], c['max_m']), end='')
    for dtype in P.DTYPES:
        terms = dtype.split('+')
        ref = P.reference(c, dtype, P.WEIGHTS, P.SCALE)
        vis, loss, dimg = host_program(c, dtype, scale=P.SCALE, weights=P.WEIGHTS, tag='%s_%d_%s' % (name, Sx, dtype))
        assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss).all()     # every element written
        assert E.rel_max(vis, c['vis']) <= E.F32_TOL
        parts = {t: float(loss[1 + P.TERMS.index(t)]) for t in terms}
        assert all(loss[1 + P.TERMS.index(t)] == 0 for t in P.TERMS if t not in terms)                             # absent terms are 0
        assert loss[0] == np.float32(loss[1] + loss[2])
        if Sx == 4:
            assert not dimg[:, 3].any() and not ref[1][:, 3].any()                                                  # the V plane: zeros
        err = P.errors(dtype, float(loss[0]), parts, dimg, ref)
        print('\n[pol, host build] %s Sx %d %-7s %s' % (name, Sx, dtype, '  '.join('%s %.1e' % kv for kv in err.items())), end='')
        for t in terms:
            assert err[t] <= bound([t]), (dtype, t, err)
        assert err['total'] <= bound(terms) and err['dimages'] <= bound(terms), (dtype, err)
        # forward only: the same loss, the same visibilities
        vis0, loss0, none = host_program(c, dtype, want_grad=False, scale=P.SCALE, weights=P.WEIGHTS, tag='nograd')
        assert none is None and loss0.tobytes() == loss.tobytes() and vis0.tobytes() == vis.tobytes()
    print()


def test_host_build_terms_alone_zero_intensity_and_infinite_sigma(host_program):
    c = P.case('12x20', 3)
    _, both, _ = host_program(c, 'pvis+m', tag='both')
    for t in P.TERMS:                                                   # a term alone at weight 1 is its value in the combined call
        _, alone, _ = host_program(c, t, tag='alone')
        assert alone[1 + P.TERMS.index(t)] == both[1 + P.TERMS.index(t)] == alone[0]
    # scale 2, weight 1 and scale 1, weight 2: one effective scale, the same bits
    _, la, da = host_program(c, 'pvis+m', scale=2.0, tag='s2')
    _, lb, db = host_program(c, 'pvis+m', scale=1.0, weights={'pvis': 2.0, 'm': 2.0}, tag='w2')
    assert la.tobytes() == lb.tobytes() and da.tobytes() == db.tobytes()
    # a frame whose I plane is exactly zero: 'm' contributes 0 there and no gradient, nothing is NaN
    z = dict(c, images=c['images'].copy())
    z['images'][0, 0] = 0.0
    vis, loss, dimg = host_program(z, 'm', tag='zero')
    _, lfull, dfull = host_program(c, 'm', tag='full')
    assert not vis[0, 0].any() and np.isfinite(loss).all() and not dimg[0].any() and np.array_equal(dimg[1:], dfull[1:]) and 0 < loss[2] < lfull[2]
    # sigma = +inf: exactly no loss and no gradient from those entries, whatever finite target stands there
    rng = np.random.default_rng(0)
    off = rng.uniform(size=c['data']['m'][1].shape) < 1.0 / 3.0
    res = []
    for shift in (0.0, 3.0 - 2.0j):
        data = {t: (np.where(off, tg + np.complex64(shift), tg), np.where(off, np.float32(np.inf), sg)) for t, (tg, sg) in c['data'].items()}
        res.append(host_program(dict(c, data=data), 'pvis+m', tag='inf'))
    assert res[0][1].tobytes() == res[1][1].tobytes() and np.array_equal(res[0][2], res[1][2]) and np.isfinite(res[0][2]).all()
    assert 0 < res[0][1][0] < both[0]


@pytest.mark.parametrize('name,Sx', P.PARAMS)
def test_mutants_of_the_reference_stand_out(name, Sx):
    """Four wrong variants of the float64 reference differ from it in dimages by more than five times the bound the device is
    held to: the bound can tell them apart."""
    c = P.case(name, Sx)
    need = 5.0 * P.bound(['m'], 'dimages')
    assert need <= 5e-3
    for dtype in ('m', 'pvis+m'):
        ref = P.reference(c, dtype, P.WEIGHTS, P.SCALE)
        for mutant in P.MUTANTS:
            if mutant == 'plane 3 <- plane 2' and Sx != 4:
                continue                                                 # (three planes have no plane 3)
            bad = P.reference(c, dtype, P.WEIGHTS, P.SCALE, mutant)
            diff = E.rel_max(bad[1], ref[1])
            print('\n[pol] %s Sx %d %-7s mutant %-20s dimages differ by %.2e' % (name, Sx, dtype, mutant, diff), end='')
            assert diff > need, (dtype, mutant, diff)
    ref = P.reference(c, 'pvis', P.WEIGHTS, P.SCALE)                      # 'pvis' alone: the mutants that touch it
    for mutant in ('P = Q - iU', 'conj target'):
        assert E.rel_max(P.reference(c, 'pvis', P.WEIGHTS, P.SCALE, mutant)[1], ref[1]) > 5.0 * E.F32_TOL, mutant
    print()


def test_sigmas_against_noise_draws(eht2017):
    """4000 noise draws on four stations held at one instant, SNR >= 20 on I: the per-component spread of the fractional
    polarisation of the noisy visibilities against the sigma that Observation.data quotes for the noise-free ones (the method of
    test_closure_sigmas_and_debiasing_against_noise_draws, its 6 % bound); the 'pvis' sigma is sqrt(2) sigma."""
    ndraw = 4000
    four = observation.Array(eht2017.names[:4], eht2017.xyz[:4], eht2017.sefd[:4])
    obs = observation.empty_eht_obs(four, ndraw, 60.0, timetype='GMST', times=np.full(ndraw, 21.0), elev_min=-91.0, elev_max=91.0)
    assert obs.up.all() and obs.nvis == 6
    snr = np.array([20.0, 24.0, 30.0, 22.0, 40.0, 26.0])                              # of I per baseline, at least 20
    vI = snr * obs.sigma[0] * np.exp(1j * np.array([0.3, -1.1, 2.0, 0.7, -2.5, 1.4]))
    vQ = vI * np.array([0.3, 0.1, -0.6, 0.8, 0.2, -0.4]) * np.exp(1j * np.array([1.0, 0.2, -0.7, 2.1, 0.0, -1.9]))
    vU = vI * np.array([-0.2, 0.7, 0.5, 0.9, -0.1, 0.3]) * np.exp(1j * np.array([-0.4, 1.3, 0.9, -2.2, 0.6, 0.1]))
    truth = np.broadcast_to(np.stack([vI, vQ, vU]), (ndraw, 3, 6))
    quoted = obs.data(truth, 'pvis+m', debias=False)
    assert quoted['triangles'] is None and quoted['quadrangles'] is None
    op = obs.pol_dft(1e-10, 8)
    assert np.abs(quoted['m'][0] - op.fractional_polarisation(truth)).max() <= 1e-12
    assert np.abs(quoted['pvis'][1] / (np.sqrt(2.0) * obs.sigma) - 1).max() <= 1e-12
    assert np.array_equal(quoted['pvis'][0], op.polarised_visibility(truth))
    m0 = np.abs(quoted['m'][0][0])
    assert np.abs(quoted['m'][1][0] / (obs.sigma[0] * np.sqrt(2 + m0 ** 2) / np.abs(vI)) - 1).max() <= 1e-12 and m0.max() > 1.0
    noisy = obs.add_thermal_noise(truth, seed=11).astype(np.complex128)
    resid = op.fractional_polarisation(noisy) - quoted['m'][0]
    resid_p = op.polarised_visibility(noisy) - quoted['pvis'][0]
    for k in range(6):
        for what, r, formula in (('m', resid[:, k], quoted['m'][1][0, k]), ('pvis', resid_p[:, k], quoted['pvis'][1][0, k])):
            for comp, got in (('re', r.real.std()), ('im', r.imag.std())):
                print('\n[observation] %s baseline %d %s: empirical sigma %.5g, formula %.5g (%.1f %%)' % (what, k, comp, got, formula,
                                                                                                          100 * (got / formula - 1)), end='')
                assert abs(got / formula - 1) <= 0.06
    # debiasing enters through |I| only
    deb = obs.data(truth, 'm')['m'][1]
    want = obs.sigma * np.sqrt(2 + np.abs(quoted['m'][0]) ** 2) / np.sqrt(np.abs(truth[:, 0]) ** 2 - obs.sigma ** 2)
    assert np.abs(deb / want - 1).max() <= 1e-12 and (deb > quoted['m'][1]).all()
    print()


def test_unobserved_baselines_and_zero_intensity_carry_no_weight(track):
    obs = track
    vis = _stokes_vis(obs)
    assert np.abs(vis[:, 0]).min() > 10 * obs.sigma.max() and (~obs.up).any() and obs.up.any()
    vis = vis.copy()
    f, k = np.argwhere(obs.up)[3]
    vis[f, 0, k] = 0.0                                                   # an observed baseline with I exactly zero
    data = obs.data(vis, 'pvis+m')
    ok = obs.up.copy()
    for term in P.TERMS:
        target, sigma = data[term]
        assert target.shape == sigma.shape == obs.up.shape and np.iscomplexobj(target) and np.isfinite(target).all()
        assert np.isposinf(sigma[~obs.up]).all() and (target[~obs.up] == 0).all()
    ok[f, k] = False
    assert np.isposinf(data['m'][1][f, k]) and data['m'][0][f, k] == 0 and np.isfinite(data['pvis'][1][f, k]) and data['pvis'][0][f, k] != 0
    assert np.isfinite(data['m'][1][ok]).all() and (data['m'][1][ok] > 0).all() and (data['m'][0][ok] != 0).all()
    # a baseline that debiasing takes to zero amplitude
    weak = vis.copy()
    weak[f, 0, k] = 0.5 * obs.sigma[f, k]
    assert np.isposinf(obs.data(weak, 'm')['m'][1][f, k]) and np.isfinite(obs.data(weak, 'm', debias=False)['m'][1][f, k])
    # four planes: V is ignored
    four = obs.data(np.concatenate([vis, vis[:, :1]], axis=1), 'pvis+m')
    assert np.array_equal(four['m'][0], data['m'][0]) and np.array_equal(four['pvis'][1], data['pvis'][1])


def test_station_gains_cancel_in_m_and_in_the_closure_quantities(track):
    obs = track
    vis = _stokes_vis(obs)
    gains = observation.station_gains(obs, seed=3)
    n = np.random.default_rng(3).standard_normal((12, 8, 2))
    assert gains.dtype == np.complex128 and gains.shape == (12, len(obs.array)) == (12, 8)
    assert np.array_equal(gains, (1.0 + 0.1 * n[..., 0]) * np.exp(1j * np.pi * n[..., 1]))
    assert np.array_equal(observation.station_gains(obs, 0.2, 0.5, seed=3), (1.0 + 0.2 * n[..., 0]) * np.exp(0.5j * n[..., 1]))
    gained = obs.apply_gains(vis, gains)
    a, b = obs.pairs[:, 0], obs.pairs[:, 1]
    assert gained.dtype == np.complex128 and np.array_equal(gained, vis * (gains[:, a] * np.conj(gains[:, b]))[:, None, :])
    assert np.array_equal(obs.apply_gains(vis[:, 0], gains), gained[:, 0])                           # without a Stokes axis
    op = obs.pol_dft(1e-10, 8)
    m, mg = op.fractional_polarisation(vis), op.fractional_polarisation(gained)
    assert np.abs(mg - m).max() <= 1e-12 * np.abs(m).max() and np.abs(mg / m - 1).max() <= 1e-12
    ns = len(obs.array)
    cl = observation.ClosureDFT(obs.uv, 1e-10, 8, pairs=obs.pairs, triangles=observation.closure_triangles(ns),
                                quadrangles=observation.closure_quadrangles(ns))
    cp, cpg = cl.closure_phases(vis[:, 0]), cl.closure_phases(gained[:, 0])
    lca, lcag = cl.log_closure_amplitudes(vis[:, 0]), cl.log_closure_amplitudes(gained[:, 0])
    assert np.abs(np.angle(np.exp(1j * (cpg - cp)))).max() <= 1e-12 * np.abs(cp).max()
    assert np.abs(lcag - lca).max() <= 1e-12 * np.abs(lca).max()
    # the calibrated terms move by the order of the gain errors (amplitudes alone: no phase errors)
    amp_only = obs.apply_gains(vis, observation.station_gains(obs, amp_sigma=0.1, phase_sigma=0.0, seed=3))
    for dtype, pick in (('vis', lambda v: obs.data(v[:, 0], 'vis')['vis'][0]), ('pvis', lambda v: obs.data(v, 'pvis')['pvis'][0])):
        t0, t1 = pick(vis)[obs.up], pick(amp_only)[obs.up]
        moved = np.median(np.abs(t1 - t0) / np.abs(t0))
        print('\n[observation] %s targets move by %.3f (median, relative) under 10 %% amplitude gains' % (dtype, moved), end='')
        assert 0.03 <= moved <= 0.3
    assert np.abs(obs.data(amp_only, 'm')['m'][0] - obs.data(vis, 'm')['m'][0]).max() <= 1e-12 * np.abs(m).max()
    with pytest.raises(AttributeError):
        obs.apply_gains(vis, gains[:, :7])
    # observe_same's host path: gains=None changes no bit; gains act on the clean visibilities, before the noise
    v64 = vis.astype(np.complex64)
    assert observation.observe_host(v64, obs, True, 5).tobytes() == obs.add_thermal_noise(v64, 5).tobytes()
    assert observation.observe_host(v64, obs, True, 5, gains=None).tobytes() == obs.add_thermal_noise(v64, 5).tobytes()
    assert observation.observe_host(v64, obs, False).tobytes() == np.where(obs.up[:, None, :], v64, 0.0).astype(np.complex64).tobytes()
    assert observation.observe_host(v64, obs, True, 5, gains).tobytes() == obs.add_thermal_noise(obs.apply_gains(v64, gains), 5).tobytes()
    clean = observation.observe_host(v64, obs, False, gains=gains)
    assert clean.dtype == np.complex64 and (clean[:, :, ~obs.up[0]][0] == 0).all()
    import inspect
    assert list(inspect.signature(observation.observe_same).parameters)[-1] == 'gains'
    assert inspect.signature(observation.observe_same).parameters['gains'].default is None
    print()


def test_pack_split_take_and_to():
    import torch
    c = P.case('12x20', 3)
    op = P.operator(c, weights={'m': 0.5})
    assert isinstance(op, observation.DirectDFT) and op.nvis == 10 and op.ncp == 0 and op.weights == {'pvis': 1.0, 'm': 0.5}
    assert observation.POL_TERMS == ('pvis', 'm')
    vis = c['vis']
    pv, m = op.polarised_visibility(vis), op.fractional_polarisation(vis)
    assert pv.dtype == m.dtype == np.complex128 and pv.shape == m.shape == (3, 10)
    assert np.array_equal(pv, vis[:, 1] + 1j * vis[:, 2]) and np.abs(m - pv / vis[:, 0]).max() <= 1e-15
    both = op.pack({'m': m, 'pvis': pv})                                 # the canonical order, whatever the dict's
    assert both.shape == (3, 20) and np.array_equal(both[:, :10], pv) and np.array_equal(both[:, 10:], m)
    back = op.split(both)
    assert list(back) == ['pvis', 'm'] and np.array_equal(back['pvis'], pv) and np.array_equal(back['m'], m)
    assert list(op.split(both, 'pvis+m')) == ['pvis', 'm'] and np.array_equal(op.split(op.pack({'m': m}), 'm')['m'], m)
    tgt, sig = P.packed(c, 'pvis+m')
    assert np.array_equal(op.pack({t: c['data'][t][0] for t in P.TERMS}), tgt) and np.array_equal(op.split(sig)['m'], c['data']['m'][1])
    for bad in (lambda: op.split(m), lambda: op.split(both, 'm'), lambda: op.split(both[:, :19]), lambda: op.pack({'vis': m}), lambda: op.pack({}),
                lambda: op.pack({'m': m[:, :9]}), lambda: op.fractional_polarisation(vis[:, :2]), lambda: op.polarised_visibility(vis[0, 0]),
                lambda: observation.PolDFT(c['uv'], E.FOV, 8, weights={'m': -1.0}), lambda: observation.PolDFT(c['uv'], E.FOV, 8, weights={'amp': 1.0})):
        with pytest.raises(AttributeError):
            bad()
    sub = op.take([2, 0])
    assert type(sub) is observation.PolDFT and sub.shape == (2, 10, 2) and sub.uv.tobytes() == c['uv'][[2, 0]].tobytes() and sub.weights == op.weights
    moved = op.to('cpu')
    assert type(moved) is observation.PolDFT and isinstance(moved.uv, torch.Tensor) and moved.uv.dtype == torch.float64 and moved.weights == op.weights
    assert type(moved.take(torch.tensor([1]))) is observation.PolDFT


def test_pol_terms_parses_the_canonical_order_only():
    from bhnerf_amd import engine
    for d in P.DTYPES:
        assert engine.pol_terms(d) == tuple(d.split('+'))
    for bad in ('vis', 'm+pvis', 'pvis+pvis', 'm+m', '', 'm+', '+m', 'pvis+m+amp', 'cphase+m', 'pvis + m', None, 3):
        assert engine.pol_terms(bad) is None, bad
    assert engine.EHT_DTYPES == {'vis': 0, 'amp': 1, 'cphase': 2} and engine.closure_terms('m') is None


def test_trainstep_eht_obs_routes_the_polarimetric_dtypes(track):
    """The host side of TrainStep.eht_obs: 'pvis', 'm' and 'pvis+m' become the TrainStep.eht_pol step (a PolDFT, the terms packed
    in the canonical order, complex64 targets); the existing dtypes keep their routes."""
    from bhnerf_amd import optimization, units
    obs = track
    vis = _stokes_vis(obs)
    t_frames = np.linspace(0.0, 0.5, 12) * units.hr
    for dtype in P.DTYPES:
        step = optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, (16, 12), dtype, weights={'m': 0.5}, scale=2.0)
        target, sigma, op = step.args[0].host_args
        data = obs.data(vis, dtype)
        assert step.num_losses == 1 and step.dtype[0] == dtype and float(step.scale[0]) == 2.0
        assert type(op) is observation.PolDFT and op.weights == {'pvis': 1.0, 'm': 0.5} and (op.H, op.W) == (16, 12) and np.array_equal(op.uv, obs.uv)
        assert target.dtype == np.complex64 and sigma.dtype == np.float32 and target.shape == sigma.shape == (12, obs.nvis * len(dtype.split('+')))
        assert np.isposinf(sigma).any()
        for term, part in op.split(sigma, dtype).items():
            assert np.array_equal(part, data[term][1].astype(np.float32))
            assert np.array_equal(op.split(target, dtype)[term], data[term][0].astype(np.complex64))
        got = step.args[0][[2, 0]][2]
        assert type(got) is observation.PolDFT and got.shape == (2, obs.nvis, 2)
    assert type(optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, 'vis').args[0].host_args[2]) is observation.DirectDFT
    assert type(optimization.TrainStep.eht_obs(t_frames, obs, vis[:, 0], 1e-10, 16, 'cphase+logcamp').args[0].host_args[2]) is observation.ClosureDFT
    both = optimization.TrainStep.eht_obs(t_frames, obs, vis[:, 0], 1e-10, 16, 'cphase+logcamp') + optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, 'm')
    assert both.num_losses == 2 and list(both.dtype) == ['cphase+logcamp', 'm']
    direct = optimization.TrainStep.eht_pol(t_frames, obs.uv, 1e-10, 16, {'m': (np.zeros((12, obs.nvis), dtype=np.complex64), 0.1)})
    assert np.all(direct.args[0].host_args[1] == np.float32(0.1))
    for bad in ({'vis': (0, 1)}, {}, {'m': (np.zeros((12, 3, obs.nvis)), 1.0)}):
        with pytest.raises(AttributeError):
            optimization.TrainStep.eht_pol(t_frames, obs.uv, 1e-10, 16, bad)


def test_mixed_families_and_too_few_planes_are_errors(track):
    import torch
    from bhnerf_amd import engine, network, optimization, units
    obs = track
    vis = _stokes_vis(obs)
    t_frames = np.linspace(0.0, 0.5, 12) * units.hr
    for dtype in ('cphase+m', 'amp+pvis', 'vis+m', 'pvis+logcamp'):
        with pytest.raises(AttributeError, match=r'TrainStep\.__add__'):
            obs.data(vis, dtype)
        with pytest.raises(AttributeError, match=r'TrainStep\.__add__'):
            optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, dtype)
    for dtype in ('m+pvis', 'm+m', 'm+nope'):
        with pytest.raises(AttributeError):
            obs.data(vis, dtype)
    for few in (vis[:, :2], vis[:, 0]):                                  # S < 3, no Stokes axis
        for dtype in P.DTYPES:
            with pytest.raises(AttributeError):
                obs.data(few, dtype)
            with pytest.raises(AttributeError):
                optimization.TrainStep.eht_obs(t_frames, obs, few, 1e-10, 16, dtype)
    with pytest.raises(AttributeError, match='should be'):               # the existing message for unknown dtypes stays
        obs.data(vis, 'nope')
    # engine and network: the polarimetric dtypes need a PolDFT, a PolDFT takes nothing else; every refusal before any launch
    c = P.case('12x20', 3)
    img = torch.as_tensor(c['images'])
    tgt, sig = P.packed(c, 'pvis+m')
    pol = P.operator(c)
    for A in (E.operator(c, 'amp'), E.operator(c, 'amp').dense()):
        for dtype in P.DTYPES:
            with pytest.raises(AttributeError, match='not supported'):
                network.test_eht(None, units.hr, dtype, tgt, sig, A, *([None] * 10), 1.0)
            with pytest.raises(AttributeError, match='not supported'):
                network.gradient_step_eht(None, units.hr, dtype, tgt, sig, A, *([None] * 10), 1.0)
    with pytest.raises(AttributeError):
        engine.chi2_eht(img, E.operator(c, 'amp'), tgt, sig, 1.0, 'pvis+m')
    for dtype in ('vis', 'amp', 'm+pvis', 'cphase+m', 'nope'):
        with pytest.raises(AttributeError, match='not supported'):
            engine.chi2_eht(img, pol, tgt, sig, 1.0, dtype)
    with pytest.raises(AttributeError, match='not supported'):
        network.test_eht(None, units.hr, 'm+pvis', tgt, sig, pol, *([None] * 10), 1.0)
    with pytest.raises(AttributeError, match='should be'):               # the last axis
        engine.chi2_eht(img, pol, tgt[:, :19], sig[:, :19], 1.0, 'pvis+m')
    with pytest.raises(AttributeError, match='should be'):
        engine.chi2_eht(img, pol, tgt, sig, 1.0, 'm')
    with pytest.raises(AttributeError, match='should be'):               # one target per frame and baseline, not per plane
        engine.chi2_eht(img, pol, np.stack([tgt] * 3, 1), np.stack([sig] * 3, 1), 1.0, 'pvis+m')
    with pytest.raises(AttributeError, match='3 or 4 planes'):           # two Stokes planes
        engine.chi2_eht(img[:, :2], pol, tgt, sig, 1.0, 'pvis+m')
    with pytest.raises(AttributeError):                                  # frame count
        engine.chi2_eht(img[:2], pol, tgt, sig, 1.0, 'pvis+m')
    with pytest.raises(AttributeError):                                  # image size
        engine.chi2_eht(img[..., :19], pol, tgt, sig, 1.0, 'pvis+m')


def test_argument_validation_returns_before_any_device_call():
    import ctypes as C
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.pol_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    N, Sx, nvis, H, W = 6, 3, 10, 12, 20
    need = lib.bhn_pol_ws_bytes(N, nvis, H, W)
    assert need > 0 and need % 256 == 0 and need > _hip.eht_lib().bhn_eht_ws_bytes(N, nvis, 0, H, W)
    for bad in ((0, nvis, H, W), (N, 0, H, W), (N, nvis, 0, W), (N, nvis, H, -1)):
        assert lib.bhn_pol_ws_bytes(*bad) == 0
    term = lambda **kw: _hip.bhn_pol_term(**dict(dict(target=4096, sigma=4096, weight=1.0), **kw))
    good = dict(images=p, uv=p, N=N, Sx=Sx, nvis=nvis, H=H, W=W, psize_x=1e-11, psize_y=1e-11, pvis=term(), m=term(), scale=1.0, loss=p,
                dimages=p, ws=p, ws_bytes=need)
    order = list(good)
    bad = [(dict(images=None), b'null', 1), (dict(uv=None), b'null', 1), (dict(loss=None), b'null', 1), (dict(ws=None), b'null', 1),
           (dict(pvis=None, m=None), b'no term present', 1), (dict(pvis=term(target=None)), b"'pvis' with a null", 1),
           (dict(m=term(sigma=None)), b"'m' with a null", 1), (dict(m=term(weight=-0.5)), b'weight', 1),
           (dict(pvis=term(weight=float('inf'))), b'weight', 1), (dict(m=term(weight=float('nan'))), b'weight', 1),
           (dict(Sx=2), b'Sx must be 3 or 4', 1), (dict(Sx=1), b'Sx must be 3 or 4', 1), (dict(Sx=5), b'Sx must be 3 or 4', 1),
           (dict(Sx=0), b'Sx must be 3 or 4', 1), (dict(Sx=4), b'multiple of Sx', 1), (dict(N=0), b'sizes below 1', 1),
           (dict(nvis=0), b'sizes below 1', 1), (dict(H=0), b'sizes below 1', 1), (dict(W=-2), b'sizes below 1', 1),
           (dict(psize_x=0.0), b'pixel sizes', 1), (dict(psize_y=float('nan')), b'pixel sizes', 1),
           (dict(ws=C.c_void_p(4100)), b'aligned', 1), (dict(uv=C.c_void_p(4100)), b'aligned', 1),
           (dict(ws_bytes=need - 1), b'workspace of', _hip.BHN_EWORKSPACE), (dict(ws_bytes=0), b'workspace of', _hip.BHN_EWORKSPACE)]
    for change, word, code in bad:
        a = dict(good, **change)
        args = [C.byref(a[k]) if isinstance(a[k], _hip.bhn_pol_term) else a[k] for k in order]
        rc = lib.bhn_pol_chi2(*args, None)
        assert rc == code, (change, rc, lib.bhn_pol_last_error())
        msg = lib.bhn_pol_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_pol'):
            _hip.pol_check(rc)
    _hip.pol_check(0)


POL_NAMES = ['bhn_pol_chi2', 'bhn_pol_last_error', 'bhn_pol_ws_bytes']


def test_pol_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_pol.so: the dynamic symbol table is the declarations of include/bhnerf_pol.h and nothing else, the ctypes table
    binds exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or
    ctypes table knows a name that begins with bhn_pol.  The ninth library has a tuple of its own: _hip.LIBRARIES keeps its five
    keys, and libbhnerf_eht.so and libbhnerf_cls.so keep their symbols."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_pol.h'))))
    assert declared == sorted(_hip.POL_SIGNATURES) == POL_NAMES
    defined = side._symbols(_hip.POL_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.POL_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.POL_LIBRARY == (_hip.POL_LIB_PATH, _hip.POL_SIGNATURES, 'bhn_pol_last_error', None)
    assert len(_hip.POL_LIBRARY) == len(_hip.CLS_LIBRARY) and [type(v) for v in _hip.POL_LIBRARY] == [type(v) for v in _hip.CLS_LIBRARY]
    assert _hip.pol_lib() is _hip.load(_hip.POL_LIB_PATH, _hip.POL_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    others += [('bhnerf_flow.h',) + _hip.FLOW_LIBRARY[:2], ('bhnerf_rec.h',) + _hip.REC_LIBRARY[:2], ('bhnerf_cls.h',) + _hip.CLS_LIBRARY[:2]]
    assert len(others) == 8
    for other_header, path, table in others:
        assert 'bhn_pol' not in side._header(other_header), other_header
        assert 'bhn_pol' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_pol') for k in table), other_header
    for path, table in ((_hip.EHT_LIB_PATH, _hip.EHT_SIGNATURES), (_hip.CLS_LIB_PATH, _hip.CLS_SIGNATURES)):
        syms = side._symbols(path, '--defined-only')
        assert sorted(line.split()[-1] for line in syms.splitlines() if line.strip()) == sorted(table)
