"""GPU tests of the equatorial crossings on the device (bhn_eql_crossings of libbhnerf_eql.so, csrc/equatorial.hip;
geodesics.equatorial_crossings, emission.equatorial_ring and kgeo.equatorial_lensing with backend='hip').

Device against host.  The kernel restates geodesics._integrate_crossings step for step, on the RK4 step it shares with the tracer, so the
two differ by rounding only (the device's sin / cos, s * s * s for s ** 3, cos / sin for 1 / tan); the bound is the tracer's, GR_TOL =
1e-10 of each row's largest magnitude over the grid (tests/test_gpu_kerr_trace.py), on the same three 70-ray grids, and `count` and the
NaN pattern are equal exactly: tests/test_equatorial_cpu.py checks that these grids keep every ray 1e-6 away from the two decisions
rounding could turn.  Closed forms: the checks of tests/test_equatorial_cpu.py on the DEVICE's output, same rays, same bounds.
Independence, reproducibility, the step budget, and the two users of the primitive.  The per-row maxima are printed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import equatorial_cases as EC                                          # noqa: E402
from bhnerf_amd import emission, geodesics as G, kgeo                  # noqa: E402
from gpu_support import dev  # noqa: F401,E402
from guarded import Guarded                                          # noqa: E402

pytestmark = pytest.mark.gpu

INC60 = np.deg2rad(60.0)


def device_crossings(dev, alpha, beta, spin, inc, nmax=EC.NMAX):
    return G._crossings_hip(alpha, beta, spin, inc, 1000.0, 1.0, EC.H, EC.R_C, EC.MAX_STEPS, nmax, dev)


@pytest.mark.parametrize('case', list(EC.GRID_CASES))
def test_crossings_equal_the_host_back_end(dev, case):
    spin, inc = EC.GRID_CASES[case]
    alpha, beta = EC.grid_rays()
    want, want_count, lam, eta = EC.host_crossings(spin, inc)
    cross, count, lam_d, eta_d = device_crossings(dev, alpha, beta, spin, inc)
    assert cross.shape == (7, 70, EC.NMAX) and cross.dtype == np.float64 and count.dtype == np.int32
    assert np.array_equal(lam_d, lam) and np.array_equal(eta_d, eta)                       # the same NumPy expressions
    assert np.array_equal(count, want_count)
    errs = EC.row_errors(cross, want)                                                        # (asserts the NaN pattern)
    print('\n[equatorial crossings, device vs host] %-20s %d crossings on 70 rays: ' % (case, count.sum())
          + '  '.join('%s %.1e' % (k, e) for k, e in zip(EC.ROWS, errs)))
    assert errs.max() <= EC.GR_TOL, (case, dict(zip(EC.ROWS, errs)))
    # and through the public function: the record of the host back end, signs included
    rec, rec_host = G.equatorial_crossings(alpha, beta, spin, inc, backend='hip', device=dev), G.equatorial_crossings(alpha, beta, spin, inc)
    assert list(rec) == list(rec_host)
    assert np.array_equal(rec.mino, -cross[0], equal_nan=True) and np.array_equal(rec.r, cross[1], equal_nan=True) and np.array_equal(rec.count, count)


def test_two_launches_a_subset_and_a_smaller_nmax_give_the_same_bytes(dev):
    spin, inc = EC.GRID_CASES['spin 0.94 / 60 deg']
    alpha, beta = EC.grid_rays()
    cross, count, _, _ = device_crossings(dev, alpha, beta, spin, inc)
    cross2, count2, _, _ = device_crossings(dev, alpha, beta, spin, inc)
    assert cross.tobytes() == cross2.tobytes() and count.tobytes() == count2.tobytes()
    sub = slice(5, 13)                                                  # rays 5..12 alone: other lanes, another n, the same bytes
    cross_s, count_s, _, _ = device_crossings(dev, alpha[sub], beta[sub], spin, inc)
    assert cross_s.shape == (7, 8, EC.NMAX)
    assert cross_s.tobytes() == np.ascontiguousarray(cross[:, sub]).tobytes() and np.array_equal(count_s, count[sub])
    k = int(np.argmax(count))                                           # one ray alone, the one with the most crossings
    cross_k, count_k, _, _ = device_crossings(dev, alpha[k:k + 1], beta[k:k + 1], spin, inc)
    assert count[k] >= 2 and cross_k.tobytes() == np.ascontiguousarray(cross[:, k:k + 1]).tobytes() and count_k[0] == count[k]
    one, count1, _, _ = device_crossings(dev, alpha, beta, spin, inc, nmax=1)
    assert one.tobytes() == np.ascontiguousarray(cross[:, :, :1]).tobytes() and np.array_equal(count1, np.minimum(count, 1))


@pytest.mark.parametrize('nmax', [3, 1])
def test_guard_bands_stay_intact_and_every_output_element_is_written(dev, nmax):
    """The caller-owned-buffer contract, as tests/test_gpu_kerr_trace.py checks it for the tracer: exactly the documented bytes between
    two guard bands, pre-filled with 0xFF (a NaN with another bit pattern than the kernel's; -1) and with 0x7F."""
    from bhnerf_amd import _hip
    spin, inc = EC.GRID_CASES['spin 0.94 / 60 deg']
    alpha, beta = EC.grid_rays()
    n = alpha.size
    a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
    results = {}
    for fill in (0xFF, 0x7F):
        bufs = [Guarded('cross', 8 * 7 * n * nmax, fill, dev), Guarded('count', 4 * n, fill, dev), Guarded('status', 4 * n, fill, dev)]
        _hip.eql_check(_hip.eql_lib().bhn_eql_crossings(_hip.ptr(a_d), _hip.ptr(b_d), n, spin, inc, 1000.0, 1.0, EC.H, EC.R_C, EC.MAX_STEPS, nmax,
                                                        bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, _hip.stream_ptr(dev)))
        torch.cuda.synchronize(dev)
        bad = [m for m in (b.disturbed() for b in bufs) if m]
        assert not bad, 'fill 0x%02X: %s' % (fill, '; '.join(bad))
        assert torch.equal(a_d.cpu(), torch.as_tensor(alpha)) and torch.equal(b_d.cpu(), torch.as_tensor(beta))        # read-only inputs
        for b, size in zip(bufs, (8, 4, 4)):
            assert b.poisoned(size) == 0, 'fill 0x%02X: %d elements of %s were not written' % (fill, b.poisoned(size), b.label)
        results[fill] = tuple(b.mid.cpu().numpy().tobytes() for b in bufs)
    assert results[0xFF] == results[0x7F]                               # nothing depends on what the buffers held
    cross, count, _, _ = device_crossings(dev, alpha, beta, spin, inc, nmax=nmax)
    assert cross.tobytes() == results[0xFF][0] and count.tobytes() == results[0xFF][1]       # what the Python surface returns


def test_an_exhausted_step_budget_is_an_error_not_a_hang(dev):
    from bhnerf_amd import _hip
    alpha, beta = np.array([-7.0, 0.5, 3.0, 8.0]), np.array([3.0, 0.25, -4.0, 1.0])
    a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
    cross = torch.zeros((7, 4, 2), dtype=torch.float64, device=dev)
    count = torch.full((4,), 77, dtype=torch.int32, device=dev)
    status = torch.zeros((4,), dtype=torch.int32, device=dev)
    rc = _hip.eql_lib().bhn_eql_crossings(_hip.ptr(a_d), _hip.ptr(b_d), 4, 0.94, INC60, 1000.0, 1.0, EC.H, EC.R_C, 10, 2, _hip.ptr(cross),
                                          _hip.ptr(count), _hip.ptr(status), _hip.stream_ptr(dev))
    assert rc == 0, _hip.eql_lib().bhn_eql_last_error()                 # BHN_OK: the budget is reported per ray
    torch.cuda.synchronize(dev)
    assert status.cpu().tolist() == [-1, -1, -1, -1] and count.cpu().tolist() == [0, 0, 0, 0]
    assert bool(torch.isnan(cross).all())                               # every element written
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):
        G.equatorial_crossings(alpha, beta, 0.94, INC60, max_steps=10, backend='hip', device=dev)
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):               # as the host back end
        G.equatorial_crossings(alpha, beta, 0.94, INC60, max_steps=10)


@pytest.mark.parametrize('spin,inc', EC.CLOSED_FORM_CASES)
def test_crossing_times_of_the_device_match_the_published_analytic_solution(dev, spin, inc):
    """The zeros of Gralla & Lupsasca 2020, eq. 38, to 1e-9 / sqrt(eta) in Mino time, and I_r to 1e-9 of the ray's total Mino time: the
    12 rays and the bounds of tests/test_equatorial_cpu.py."""
    alpha, beta = EC.grid_rays(3, 4)
    cross, count, lam, eta = device_crossings(dev, alpha, beta, spin, inc)
    assert count.size == 12 and (eta > 1.0).all() and (count >= 1).sum() >= 8
    polar, radial, n_rays, n_cross = EC.closed_form_errors(spin, inc, cross, count, lam, eta, beta)
    print('\n[equatorial crossings, device] spin %g: polar %.2e (x sqrt(eta); %d crossings), radial %.2e of the total Mino time (%d rays, %d crossings)'
          % (spin, polar, count.sum(), radial, n_rays, n_cross))
    assert n_rays >= 4
    assert polar <= 1e-9, polar
    assert radial <= 1e-9, radial


@pytest.mark.parametrize('mbar', [0, 1])
def test_rho_of_req_on_the_device_brackets_the_requested_radius_on_the_host(dev, mbar):
    """rho from the device's bisection, judged by the HOST back end: r_cross at rho (1 - e) and rho (1 + e) straddles req with
    e = 1e-9.  Derivation: the device's r_cross is within GR_TOL req = 1e-10 req of the host's, so the two back ends' answers differ
    by at most that over dr/drho; dr/drho >= 1 (a lensing band is never wider than the stretch of the plane it shows), so
    |d rho| <= 1e-10 req <= 1e-10 rho (6 / 3.8) at these angles, and e is ten times the 1e-10."""
    EL = kgeo.equatorial_lensing
    spin, req, distance = 0.94, 6.0, 200.0
    varphis = np.deg2rad(np.linspace(5.0, 320.0, 8))
    rho, vp, alpha, beta = EL.rho_of_req(spin, INC60, req, mbar=mbar, varphis=varphis, distance=distance, backend='hip', device=dev)
    assert rho.shape == (8,) and np.array_equal(vp, varphis) and np.array_equal(alpha, rho * np.cos(varphis))
    e = 1e-9
    inner = EL.r_equatorial(spin, distance, INC60, mbar, alpha * (1 - e), beta * (1 - e))[0]
    outer = EL.r_equatorial(spin, distance, INC60, mbar, alpha * (1 + e), beta * (1 + e))[0]
    print('\n[rho_of_req, device] mbar %d: rho %s\n    host r_cross - req at rho (1 -+ 1e-9): %s / %s' % (mbar, rho, inner - req, outer - req))
    assert (inner < req).all() and (outer > req).all()


def test_equatorial_ring_on_the_device_equals_the_host_result(dev):
    geos = G.image_plane_geos(0.94, INC60, EC.FOV, EC.FOV, ngeo=60, num_alpha=12, num_beta=12, backend='hip', device=dev)
    for mbar in (0, 1):
        ring, ring_host = emission.equatorial_ring(geos, mbar, backend='hip', device=dev), emission.equatorial_ring(geos, mbar)
        assert ring.shape == (12, 12, 60) and ring.sum() >= (100, 10)[mbar]
        assert ring.dtype == ring_host.dtype and ring.tobytes() == ring_host.tobytes()
