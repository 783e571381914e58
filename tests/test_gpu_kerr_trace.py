"""GPU tests of the Kerr tracer on the device (bhn_kerr_trace of libbhnerf_kerr.so, csrc/kerr_trace.hip; geodesics.trace / image_plane_geos with
backend='hip').

Device against host.  The kernel restates geodesics._integrate step for step, so the two differ by rounding only (the device's
sin / cos, s * s * s for s ** 3, cos / sin for 1 / tan).  Rounding-size noise on every right-hand-side evaluation moves the sampled
rows of these grids by <= 5e-12 of the row's largest magnitude, a one-ulp change of (alpha, beta) by <= 8e-13; the bound is the
project's GR_TOL = 1e-10 (tests/test_geodesics_cpu.py), 20 times that: each of the seven rows (mino, r, theta, phi, t, vr, vth), end
states and samples, relative to the row's largest magnitude over the grid.  The derived fields of the Geodesics record (x, y, z, Delta,
Sigma, Xi, omega, R, Theta, dtau, affine) come out of the same NumPy code on both sides, from rows that agree that well; they are smooth
in the rows, and measured against their own largest magnitude -- which Theta, R and omega reach exactly where they are steepest, next to
the pole and next to the horizon -- a row difference is amplified by a factor of order 1 to 10, so rows at the expected 1e-12 keep them
inside the same 1e-10.  The per-row maxima are printed.  MEASURED on the MI355X: see DESIGN.md 4.9.

Closed forms: the radial (Gralla & Lupsasca I_r) and polar (Jacobi sn) checks of tests/test_geodesics_cpu.py on the DEVICE's output, at
that file's bounds.  Independence, reproducibility, the caller-owned-buffer contract (guard bands, poisoned outputs, in the style of
tests/test_gpu_buffer_contract.py), the exhausted step budget, and the way through alma.get_raytracing_args into a training step."""
import numpy as np
import pytest
import torch

from bhnerf_amd import geodesics as G
from gpu_support import dev  # noqa: F401
from guarded import Guarded

pytestmark = pytest.mark.gpu

GR_TOL = 1e-10
ROWS = ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth')
H, R_C, MAX_STEPS = 0.02, 5.0, 400000
FOV = ((-9.0, 9.0), (-9.0, 9.0))

# name -> (spin, inclination, alpha_range, beta_range, num_alpha, num_beta, ngeo, distance, M, captured rays at least)
CASES = {
    'spin 0.94 / 60 deg': (0.94, np.deg2rad(60.0), FOV[0], FOV[1], 10, 7, 40, 1000.0, 1.0, 4),       # 70 rays: one wave + a 6-lane tail
    'spin 0.94 / 17 deg': (0.94, np.deg2rad(17.0), FOV[0], FOV[1], 10, 7, 40, 1000.0, 1.0, 4),       # the polar step clip
    'spin 0 / 60 deg': (0.0, np.deg2rad(60.0), FOV[0], FOV[1], 10, 7, 40, 1000.0, 1.0, 4),           # a = 0
    'flat space': (0.0, np.deg2rad(50.0), (2.0, 6.0), (-5.0, -3.0), 2, 2, 30, 200.0, 1e-9, 0),
    'edge on': (0.8, 0.5 * np.pi, (-6.0, 6.0), (-5.0, 5.0), 3, 2, 25, 1000.0, 1.0, 0),               # inclination exactly pi / 2
}


def geos_kw(case):
    spin, inc, ar, br, na, nb, ngeo, dist, M, _ = CASES[case]
    return (spin, inc, ar, br), dict(ngeo=ngeo, num_alpha=na, num_beta=nb, distance=dist, M=M)


def rays(case):
    spin, inc, ar, br, na, nb, ngeo, dist, M, _ = CASES[case]
    alpha, beta = np.meshgrid(np.linspace(*ar, na), np.linspace(*br, nb), indexing='ij')
    return alpha.ravel(), np.where(beta == 0.0, 1e-9, beta).ravel()


_HOST = {}


def host(case, what):
    """The NumPy tracer's answer, computed once per case and left unchanged: 'geos' the record, 'trace' the end states."""
    key = (case, what)
    if key not in _HOST:
        args, kw = geos_kw(case)
        if what == 'geos':
            _HOST[key] = G.image_plane_geos(*args, backend='numpy', **kw)
        else:
            _HOST[key] = G.trace(*rays(case), args[0], args[1], distance=kw['distance'], M=kw['M'], backend='numpy')
    return _HOST[key]


def rel_to_max(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    if want.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / (np.abs(want).max() or 1.0))


@pytest.mark.parametrize('case', list(CASES))
def test_end_states_equal_the_host_tracer(dev, case):
    spin, inc, ar, br, na, nb, ngeo, dist, M, ncap = CASES[case]
    alpha, beta = rays(case)
    want = host(case, 'trace')
    got = G.trace(alpha, beta, spin, inc, distance=dist, M=M, backend='hip', device=dev)
    assert len(got) == 4 and all(np.asarray(g).shape == np.asarray(w).shape and np.asarray(g).dtype == np.asarray(w).dtype for g, w in zip(got, want))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])               # lam, eta: the same NumPy expressions
    r_hor = M + np.sqrt(max(M * M - (spin * M) ** 2, 0.0))
    captured = want[1][0] < 1.2 * r_hor
    assert captured.sum() >= ncap and ((want[1][0] > dist) | captured).all()
    errs = [rel_to_max(got[0], want[0])] + [rel_to_max(got[1][k], want[1][k]) for k in range(6)]
    print('\n[kerr trace, device vs host] %-20s end states (%d rays, %d captured): ' % (case, alpha.size, captured.sum())
          + '  '.join('%s %.1e' % (k, e) for k, e in zip(ROWS, errs)))
    assert max(errs) <= GR_TOL, (case, dict(zip(ROWS, errs)))


@pytest.mark.parametrize('case', list(CASES))
def test_geodesics_record_equals_the_host_tracer(dev, case):
    args, kw = geos_kw(case)
    want = host(case, 'geos')
    got = G.image_plane_geos(*args, backend='hip', device=dev, **kw)
    assert isinstance(got, G.Geodesics) and list(got) == list(want)
    errs = {}
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        errs[k] = rel_to_max(g, w)
    for k in ('alpha', 'beta', 'lam', 'eta', 'spin', 'inc', 'M', 'E', 'r_o'):
        assert errs[k] == 0.0, k                                                              # never on the device
    rows = ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth')
    print('\n[kerr trace, device vs host] %-20s samples: ' % case + '  '.join('%s %.1e' % (k, errs[k]) for k in rows))
    print('    derived fields: ' + '  '.join('%s %.1e' % (k, e) for k, e in errs.items() if k not in rows and e > 0.0))
    assert max(errs.values()) <= GR_TOL, (case, {k: e for k, e in errs.items() if e > GR_TOL})


# ---- the closed forms of tests/test_geodesics_cpu.py on the device's output

def _gl_radial_integral(r, roots):
    """I_r(r) = int_{r4}^{r} dr / sqrt(R(r)) for four real roots r1 < r2 < r3 < r4 <= r (Gralla & Lupsasca 2020, eq. B35 / B40)."""
    import mpmath as mp
    r1, r2, r3, r4 = roots
    r31, r32, r41, r42 = r3 - r1, r3 - r2, r4 - r1, r4 - r2
    k = r32 * r41 / (r31 * r42)
    x2 = (r - r4) * r31 / ((r - r3) * r41)
    return 2 / mp.sqrt(r31 * r42) * mp.ellipf(mp.asin(mp.sqrt(x2)), k)


_CLOSED = {}


def closed_form_geos(dev, spin, inc_deg):
    key = (spin, inc_deg)
    if key not in _CLOSED:
        _CLOSED[key] = G.image_plane_geos(spin, np.deg2rad(inc_deg), FOV[0], FOV[1], ngeo=40, num_alpha=3, num_beta=4, backend='hip', device=dev)
    return _CLOSED[key]


@pytest.mark.parametrize('spin,inc_deg', [(0.94, 60.0), (0.0, 60.0)])
def test_radial_motion_of_the_device_rays_matches_the_analytic_solution(dev, spin, inc_deg):
    """Mino time elapsed since the observer = I_r(r_o) -+ I_r(r) before / after the radial turning point, to 1e-9 of the ray's total
    Mino time (mpmath, 30 digits), on at least 6 scattering rays."""
    import mpmath as mp
    mp.mp.dps = 30
    g = closed_form_geos(dev, spin, inc_deg)
    err, n_rays = 0.0, 0
    for i in range(3):
        for j in range(4):
            lam, eta, a = float(g.lam[i, j]), float(g.eta[i, j]), spin
            roots = mp.polyroots([1, 0, a * a - eta - lam * lam, 2 * (eta + (lam - a) ** 2), -a * a * eta], maxsteps=200, extraprec=200)
            if any(abs(mp.im(z)) > 1e-12 for z in roots):
                continue                                       # plunging ray: two complex roots
            roots = sorted(mp.re(z) for z in roots)
            r, tau = g.r[i, j], -g.mino[i, j]
            if not np.isfinite(r).all() or r.min() < float(roots[3]) * (1 - 1e-3):
                continue
            k0 = int(np.argmin(r))
            assert abs(r[k0] - float(roots[3])) < 0.5          # the ray turns at the largest root
            I_o = _gl_radial_integral(mp.mpf(float(g.r_o)), roots)
            for k in range(len(r)):
                if k == k0:
                    continue                                   # next to the turning point: branch ambiguous
                I_k = _gl_radial_integral(mp.mpf(float(r[k])), roots)
                want = I_o - I_k if k < k0 else I_o + I_k
                err = max(err, abs(float(want) - tau[k]) / float(2 * I_o))
            n_rays += 1
    print('\n[kerr trace, device] radial closed form, spin %g: %.2e of the total Mino time over %d rays' % (spin, err, n_rays))
    assert n_rays >= 6
    assert err < 1e-9, err


@pytest.mark.parametrize('spin,inc_deg', [(0.94, 60.0), (0.0, 60.0)])
def test_polar_motion_of_the_device_rays_matches_the_analytic_solution(dev, spin, inc_deg):
    """cos theta(tau) = -nu sqrt(u_+) sn(sqrt(-u_- a^2) (tau + nu G_o) | u_+ / u_-) (Gralla & Lupsasca 2020, eq. 38) and its a -> 0
    limit, to 1e-9 in cos theta, on at least 8 rays."""
    import mpmath as mp
    mp.mp.dps = 30
    g = closed_form_geos(dev, spin, inc_deg)
    th_o = mp.mpf(float(g.inc))
    err, n_rays = 0.0, 0
    for i in range(3):
        for j in range(4):
            lam, eta, a = mp.mpf(float(g.lam[i, j])), mp.mpf(float(g.eta[i, j])), mp.mpf(spin)
            th, tau = g.theta[i, j], -g.mino[i, j]
            if eta <= 0 or not np.isfinite(th).all():
                continue
            nu = -1 if g.beta[i, j] > 0 else 1
            if a == 0:
                up, w = eta / (eta + lam ** 2), mp.sqrt(eta + lam ** 2)
                G_o = -mp.asin(mp.cos(th_o) / mp.sqrt(up)) / w
                f = lambda t: -nu * mp.sqrt(up) * mp.sin(w * (t + nu * G_o))
            else:
                D = (1 - (eta + lam ** 2) / a ** 2) / 2
                up, um = D + mp.sqrt(D ** 2 + eta / a ** 2), D - mp.sqrt(D ** 2 + eta / a ** 2)
                w, m = mp.sqrt(-um * a ** 2), up / um
                G_o = -mp.re(mp.ellipf(mp.asin(mp.cos(th_o) / mp.sqrt(up)), m)) / w
                f = lambda t: -nu * mp.sqrt(up) * mp.re(mp.ellipfun('sn', w * (t + nu * G_o), m))
            assert abs(float(f(mp.mpf(0))) - float(mp.cos(th_o))) < 1e-12
            for k in range(len(th)):
                err = max(err, abs(float(f(mp.mpf(float(tau[k])))) - np.cos(th[k])))
            n_rays += 1
    print('\n[kerr trace, device] polar closed form, spin %g: %.2e in cos theta over %d rays' % (spin, err, n_rays))
    assert n_rays >= 8
    assert err < 1e-9, err


# ---- independence and reproducibility

def test_two_launches_and_a_subset_of_the_rays_give_the_same_bytes(dev):
    case = 'spin 0.94 / 60 deg'
    spin, inc, ar, br, na, nb, ngeo, dist, M, _ = CASES[case]
    alpha, beta = rays(case)
    run = lambda sl: G._trace_hip(alpha[sl], beta[sl], spin, inc, dist, M, H, R_C, MAX_STEPS, ngeo, dev)[:2]
    end, samples = run(slice(None))
    end2, samples2 = run(slice(None))
    assert end.tobytes() == end2.tobytes() and samples.tobytes() == samples2.tobytes()
    sub = slice(5, 13)                                                  # rays 5..12 alone: other lanes, another n, the same bytes
    end_s, samples_s = run(sub)
    assert end_s.shape == (7, 8) and samples_s.shape == (7, 8, ngeo)
    assert end_s.tobytes() == np.ascontiguousarray(end[:, sub]).tobytes()
    assert samples_s.tobytes() == np.ascontiguousarray(samples[:, sub]).tobytes()


# ---- caller-owned buffers

GUARD = 1 << 16
FILLS = (0xFF, 0x7F)            # NaN as float64, -1 as int32;  1.4e306 as float64, 0x7F7F7F7F as int32


@pytest.mark.parametrize('ngeo', [40, 0])
def test_guard_bands_stay_intact_and_every_output_element_is_written(dev, ngeo):
    from bhnerf_amd import _hip
    case = 'spin 0.94 / 60 deg'
    spin, inc = CASES[case][:2]
    alpha, beta = rays(case)
    n = alpha.size
    assert n == 70
    a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
    results = {}
    for fill in FILLS:
        samples = Guarded('samples', 8 * 7 * n * ngeo, fill, dev, guard=GUARD) if ngeo else None
        end, status = Guarded('end', 8 * 7 * n, fill, dev, guard=GUARD), Guarded('status', 4 * n, fill, dev, guard=GUARD)
        rc = _hip.kerr_lib().bhn_kerr_trace(_hip.ptr(a_d), _hip.ptr(b_d), n, spin, inc, 1000.0, 1.0, H, R_C, MAX_STEPS, ngeo,
                                       samples.ptr if ngeo else None, end.ptr, status.ptr, _hip.stream_ptr(dev))
        _hip.kerr_check(rc)
        torch.cuda.synchronize(dev)
        bufs = [b for b in (samples, end, status) if b is not None]
        bad = [m for m in (b.disturbed() for b in bufs) if m]
        assert not bad, 'fill 0x%02X: %s' % (fill, '; '.join(bad))
        assert torch.equal(a_d.cpu(), torch.as_tensor(alpha)) and torch.equal(b_d.cpu(), torch.as_tensor(beta))        # read-only inputs
        for b, size in ((samples, 8), (end, 8), (status, 4)):
            if b is not None:
                assert b.poisoned(size) == 0, 'fill 0x%02X: %d elements of %s were not written' % (fill, b.poisoned(size), b.label)
        st = status.mid.cpu().numpy().view(np.int32)
        assert (st > 0).all() and (st < MAX_STEPS).all()
        results[fill] = tuple(b.mid.cpu().numpy().tobytes() for b in bufs)
    assert results[FILLS[0]] == results[FILLS[1]]                       # nothing depends on what the buffers held
    # and they hold what the Python surface returns
    end_py, samples_py = G._trace_hip(alpha, beta, spin, inc, 1000.0, 1.0, H, R_C, MAX_STEPS, ngeo, dev)[:2]
    assert end_py.tobytes() == results[FILLS[0]][-2]
    if ngeo:
        assert samples_py.tobytes() == results[FILLS[0]][0]
    else:
        assert samples_py is None


# ---- non-termination is data

def test_an_exhausted_step_budget_is_an_error_not_a_hang(dev):
    from bhnerf_amd import _hip
    alpha, beta = np.array([-7.0, 0.5, 3.0, 8.0]), np.array([3.0, 0.25, -4.0, 1.0])
    a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
    end = torch.full((7, 4), np.nan, dtype=torch.float64, device=dev)
    samples = torch.full((7, 4, 5), np.nan, dtype=torch.float64, device=dev)
    status = torch.zeros((4,), dtype=torch.int32, device=dev)
    rc = _hip.kerr_lib().bhn_kerr_trace(_hip.ptr(a_d), _hip.ptr(b_d), 4, 0.94, np.deg2rad(60.0), 1000.0, 1.0, H, R_C, 10, 5, _hip.ptr(samples),
                                   _hip.ptr(end), _hip.ptr(status), _hip.stream_ptr(dev))
    assert rc == 0, _hip.kerr_lib().bhn_kerr_last_error()                         # BHN_OK: the budget is reported per ray
    torch.cuda.synchronize(dev)
    assert status.cpu().tolist() == [-1, -1, -1, -1]
    e, s = end.cpu().numpy(), samples.cpu().numpy()
    assert np.isfinite(e).all() and (e[1] > 900.0).all() and (e[1] < 1000.0).all()          # ten steps inwards from the observer
    assert np.array_equal(s, np.repeat(e[:, :, None], 5, axis=2))
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):
        G.image_plane_geos(0.94, np.deg2rad(60.0), FOV[0], FOV[1], ngeo=5, num_alpha=2, num_beta=2, max_steps=10, backend='hip', device=dev)
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):
        G.trace(alpha, beta, 0.94, np.deg2rad(60.0), max_steps=10, backend='hip', device=dev)
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):               # as the host tracer
        G.trace(alpha, beta, 0.94, np.deg2rad(60.0), max_steps=10)


# ---- through the ALMA glue

def test_alma_raytracing_args_with_the_hip_tracer_feed_a_training_step(dev):
    from bhnerf_amd import alma, network, optimization, units
    params = dict(fov_M=40.0, z_width=4, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0, avert=1, ator=0), Omega_dir='cw',
                  num_alpha=8, num_beta=8, t_start_obs=9.3)
    rt_np = alma.get_raytracing_args(np.deg2rad(12.0), 0.0, params)
    rt = alma.get_raytracing_args(np.deg2rad(12.0), 0.0, dict(params, tracer='hip'))
    assert len(rt) == len(rt_np) == 1 and list(rt[0]) == list(rt_np[0])
    for k in rt[0]:
        assert type(rt[0][k]) is type(rt_np[0][k]), k
        g, w = np.asarray(units.strip(rt[0][k])), np.asarray(units.strip(rt_np[0][k]))
        assert g.shape == w.shape and g.dtype == w.dtype, k
        assert np.isfinite(g).all() and np.allclose(g, w, rtol=1e-6, atol=1e-6 * (np.abs(w).max() or 1.0)), k
    t = (9.3 + np.linspace(0.05, 0.5, 4)) * units.hr
    data = np.abs(np.random.default_rng(3).standard_normal((4, 3))) * 1e-2
    pred = network.NeRF_Predictor(20.0, 6.0, 20.0, 4.0, net_depth=4, net_width=64, mode='f32', device=dev)
    step = optimization.TrainStep.image(t, data, sigma=1e-2, dtype='lc')
    opt = optimization.Optimizer({'num_iters': 1, 'lr_init': 1e-3, 'lr_final': 1e-4}, pred, rt)
    opt.run(4, step, rt)
    assert opt.state.step == 1 and np.isfinite(float(np.mean(opt.loss)))
