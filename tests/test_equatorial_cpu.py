"""CPU tests of the equatorial crossings (geodesics.equatorial_crossings, bhn_eql_crossings of csrc/equatorial.hip) and of what is
built on them (geodesics.ray_geos, emission.equatorial_ring, kgeo.equatorial_lensing): everything that needs no device.

Closed forms.  The crossings of the NumPy back end against the zeros of Gralla & Lupsasca 2020, eq. 38 (Jacobi sn), and against
their radial integral I_r: an oracle independent of the tracer (tests/equatorial_cases.py; mpmath, 30 digits).  Bounds: 1e-9 / sqrt(eta)
in Mino time -- the project's polar bound, 1e-9 in cos theta (tests/test_geodesics_cpu.py), carried through the slope of cos theta at
the equator, sqrt(eta) -- and the project's radial bound, 1e-9 of the ray's total Mino time.  MEASURED (host): polar 7.6e-11 / 7.4e-11
(times sqrt(eta)) at spin 0.94 / 0 on the 12 rays; radial 1.9e-10 / 1.9e-10.  Second and third crossings: see the test of that name.

Host program.  The per-ray code lives in csrc/equatorial.h and compiles with a plain C++ compiler; tools/equatorial_host.cpp is a
stand-alone program around it, built here with g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process on output
blocks of exactly the documented size and compared with the NumPy back end: GR_TOL = 1e-10 of each row's largest magnitude, count and
NaN pattern equal.  Nothing built with a sanitizer is loaded into this Python process."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import equatorial_cases as EC                                          # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import emission, geodesics as G, kgeo                  # noqa: E402

GR_TOL = EC.GR_TOL
INC60 = np.deg2rad(60.0)
# rays (alpha, +-beta) next to the critical curve of spin 0.94 / 60 deg: two or three crossings each
NEAR_CRITICAL_ALPHA, NEAR_CRITICAL_BETA = np.array([-1.5, 4.75, 0.5, 2.75]), np.array([4.0, 4.0, 5.0, 5.0])


# ---- closed forms

@pytest.mark.parametrize('spin,inc', EC.CLOSED_FORM_CASES)
def test_crossing_times_match_the_published_analytic_solution(spin, inc):
    cross, count, lam, eta = EC.host_crossings(spin, inc, 3, 4)
    _, beta = EC.grid_rays(3, 4)
    assert count.size == 12 and (eta > 1.0).all() and (count >= 1).sum() >= 8
    polar, radial, n_rays, n_cross = EC.closed_form_errors(spin, inc, cross, count, lam, eta, beta)
    print('\n[equatorial crossings, host] spin %g: polar %.2e (x sqrt(eta); %d crossings), radial %.2e of the total Mino time (%d rays, %d crossings)'
          % (spin, polar, count.sum(), radial, n_rays, n_cross))
    assert n_rays >= 4
    assert polar <= 1e-9, polar
    assert radial <= 1e-9, radial


def test_higher_order_crossings_converge_to_the_analytic_solution_at_fourth_order():
    """Second and third crossings exist only on rays next to the critical curve, which linger near the photon shell (r = 2..3.6).
    There the RK4 TRACER's own phase error at the default step exceeds 1e-9 / sqrt(eta): MEASURED 3.9e-07 (x sqrt(eta)) at h = 0.02,
    2.3e-08 at h = 0.01, first crossings of the same rays <= 8.4e-09 -- sixteen times smaller per halving, the tracer's truncation
    error, to which the crossing search adds nothing of lower order.  That convergence is what is asserted (the bound
    1e-9 / sqrt(eta) is held on the 12 ordinary rays above); a wrongly counted crossing would be off by half a polar period,
    about 0.6, at either step."""
    alpha = np.concatenate([NEAR_CRITICAL_ALPHA, NEAR_CRITICAL_ALPHA])
    beta = np.concatenate([NEAR_CRITICAL_BETA, -NEAR_CRITICAL_BETA])
    errs = []
    for h in (0.02, 0.01):
        c = G.equatorial_crossings(alpha, beta, 0.94, INC60, nmax=3, h=h)
        assert (c.count >= 2).all() and (c.count == 3).sum() >= 4 and (c.eta > 1.0).all()
        cross = np.stack([-c.mino, c.r, c.theta, -c.phi, -c.t, c.vr, c.vth])
        errs.append(EC.closed_form_errors(0.94, INC60, cross, c.count, c.lam, c.eta, beta)[0])
    print('\n[equatorial crossings, host] near-critical rays, 22 crossings: polar %.2e at h = 0.02, %.2e at h = 0.01 (x sqrt(eta))' % tuple(errs))
    assert errs[1] < errs[0] / 8.0, errs


# ---- invariants

def test_reflection_symmetry_about_an_equatorial_observers_mirror():
    """An observer a tilt d above the plane (inclination pi/2 - d; d = 2e-6, twice what is refused) and the rays (alpha, beta),
    (alpha, -beta): the same lam and eta, so the same r(tau) and the same polar orbit.  The ray that starts downwards meets the
    plane at once, G = d / sqrt(eta) (1 + O(d^2)) after the observer (sqrt(u_+) w = sqrt(eta) exactly in eq. 38), inside the first
    RK4 step, and from there on is the mirror image of the other ray, 2 G behind it: crossing j + 1 of (alpha, -|beta|) is crossing
    j of (alpha, |beta|) at tau + 2 G, r + v_r 2 G.  Bounds: the polar bound 1e-9 / sqrt(eta) for each Mino time that enters; for r
    that times |v_r|, plus the second-order term |R'/2| (2 G)^2 and GR_TOL r for the interpolation."""
    d = 2e-6
    inc = 0.5 * np.pi - d
    alpha, beta = np.array([-6.0, -2.0, 3.0, 7.0]), np.array([3.0, 5.0, 4.0, 2.0])
    up = G.equatorial_crossings(alpha, beta, 0.8, inc, nmax=1)
    down = G.equatorial_crossings(alpha, -beta, 0.8, inc, nmax=2)
    assert (up.count == 1).all() and (down.count == 2).all() and np.array_equal(up.eta, down.eta) and np.array_equal(up.lam, down.lam)
    gap, tol = d / np.sqrt(up.eta), 1e-9 / np.sqrt(up.eta)
    # at once, next to the observer: |dr/dtau| <= r^2 = 1e6 there (R <= r^4 up to O(1/r) terms)
    assert (down.r[:, 0] >= 1000.0 - 1.001e6 * gap).all() and (down.r[:, 0] < 1000.0).all() and (np.abs(-down.mino[:, 0] - gap) <= tol).all()
    assert (np.abs((-down.mino[:, 1]) - (-up.mino[:, 0]) - 2 * gap) <= 2 * tol).all()
    r, vr = up.r[:, 0], up.vr[:, 0]
    accel = np.abs(2.0 * r * (r * r + 0.64 - 0.8 * up.lam) - (r - 1.0) * (up.eta + (up.lam - 0.8) ** 2))      # |R'(r) / 2|
    assert (np.abs(down.r[:, 1] - r - vr * 2 * gap) <= np.abs(vr) * 2 * tol + accel * (2 * gap) ** 2 + GR_TOL * r).all()
    assert (np.abs(down.theta - 0.5 * np.pi) <= 1e-12).all()


def test_crossings_lie_on_the_plane_and_keep_the_radial_constant_of_motion():
    for case, (spin, inc) in EC.GRID_CASES.items():
        cross, count, lam, eta = EC.host_crossings(spin, inc)
        found = np.arange(EC.NMAX)[None, :] < count[:, None]
        assert np.array_equal(np.isfinite(cross), np.broadcast_to(found, cross.shape)), case
        assert count.sum() >= 60 and (count >= 2).sum() >= 5
        assert np.abs(cross[2][found] - 0.5 * np.pi).max() <= 1e-12
        r, vr = cross[1], cross[5]
        R = G.radial_potential(r, spin, lam[:, None], eta[:, None])
        assert (np.abs(vr ** 2 - R) / r ** 4)[found].max() < 2e-3       # the tolerance of test_constants_of_motion_and_layout
        mino = cross[0]
        assert (np.diff(mino, axis=1)[found[:, 1:]] > 0).all() and (mino[found] > 0).all()


def test_vortical_rays_never_meet_the_plane():
    alpha, beta = np.array([-0.3, 0.1, 0.4, 0.1]), np.array([0.05, -0.05, 0.1, 0.2])
    c = G.equatorial_crossings(alpha, beta, 0.94, np.deg2rad(17.0), nmax=2)
    assert (c.eta < 0).all()
    assert c.count.tolist() == [0, 0, 0, 0] and np.isnan(c.r).all() and c.r.shape == (4, 2)


def test_record_layout_and_sign_convention():
    alpha, beta = EC.grid_rays()
    spin, inc = EC.GRID_CASES['spin 0.94 / 60 deg']
    cross, count, lam, eta = EC.host_crossings(spin, inc)
    c = G.equatorial_crossings(alpha, beta, spin, inc)                  # nmax = 3, the NumPy back end: the defaults
    assert isinstance(c, G.Geodesics) and c.r.shape == (70, 3) and c.count.dtype == np.int32
    for name, row, sign in (('mino', 0, -1), ('r', 1, 1), ('theta', 2, 1), ('phi', 3, -1), ('t', 4, -1), ('vr', 5, 1), ('vth', 6, 1)):
        assert np.array_equal(c[name], sign * cross[row], equal_nan=True), name
    assert np.array_equal(c.count, count) and np.array_equal(c.lam, lam) and np.array_equal(c.eta, eta)
    assert (c.mino[np.isfinite(c.mino)] < 0).all() and (c.t[np.isfinite(c.t)] < 0).all()
    one = G.equatorial_crossings(alpha, beta, spin, inc, nmax=1)
    assert np.array_equal(one.r[:, 0], c.r[:, 0], equal_nan=True) and np.array_equal(one.count, np.minimum(count, 1))
    with pytest.raises(RuntimeError, match='did not terminate in 10 steps'):
        G.equatorial_crossings(alpha[:4], beta[:4], spin, inc, max_steps=10)


# ---- the host program under the sanitizers

@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/equatorial_host.cpp built with the sanitizers -> a function -> (cross (7, n, nmax), count (n), status (n))."""
    exe, work = side.build_host_program(tmp_path_factory, 'equatorial_host')

    def run(alpha, beta, spin, inc, nmax, max_steps=EC.MAX_STEPS, tag='case'):
        n = alpha.size
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        np.concatenate([[n, nmax, max_steps, spin, inc, 1000.0, 1.0, EC.H, EC.R_C], alpha, beta]).astype(np.float64).tofile(fin)
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        assert len(raw) == 8 * 7 * n * nmax + 4 * n + 4 * n           # the documented sizes, nothing else
        cross = np.frombuffer(raw, dtype=np.float64, count=7 * n * nmax).reshape(7, n, nmax)
        count = np.frombuffer(raw, dtype=np.int32, count=n, offset=8 * 7 * n * nmax)
        status = np.frombuffer(raw, dtype=np.int32, count=n, offset=8 * 7 * n * nmax + 4 * n)
        return cross, count, status
    return run


@pytest.mark.parametrize('case', list(EC.GRID_CASES))
def test_host_build_of_the_crossing_code_equals_the_numpy_back_end(host_program, case):
    spin, inc = EC.GRID_CASES[case]
    alpha, beta = EC.grid_rays()
    want, want_count, _, _ = EC.host_crossings(spin, inc)
    # the grid keeps every ray away from the two decisions rounding could turn: a crossing next to the ray's end, an end on the plane
    mino_end, y_end = EC.host_ends(spin, inc)
    last = np.where(want_count > 0, want[0][np.arange(alpha.size), np.maximum(want_count - 1, 0)], -np.inf)
    assert (mino_end - last >= 1e-6).all() and (np.abs(y_end[1] - 0.5 * np.pi) > 1e-6).all()
    cross, count, status = host_program(alpha, beta, spin, inc, EC.NMAX, tag='c%d' % list(EC.GRID_CASES).index(case))
    assert (status > 0).all() and (status < EC.MAX_STEPS).all()       # every element written (0x7F7F7F7F where not), every ray finished
    assert np.array_equal(count, want_count)
    errs = EC.row_errors(cross, want)                                  # (asserts the NaN pattern)
    print('\n[equatorial crossings, host build] %-20s %d crossings on %d rays: ' % (case, count.sum(), alpha.size)
          + '  '.join('%s %.1e' % (k, e) for k, e in zip(EC.ROWS, errs)))
    assert errs.max() <= GR_TOL, (case, errs)


def test_an_exhausted_step_budget_is_reported_and_every_element_written(host_program):
    alpha, beta = np.array([-7.0, 0.5, 3.0, 8.0]), np.array([3.0, 0.25, -4.0, 1.0])
    cross, count, status = host_program(alpha, beta, 0.94, INC60, 2, max_steps=10, tag='budget')
    assert (status == -1).all() and (count == 0).all() and np.isnan(cross).all()
    # nmax = 1 stops a lane at its first crossing: column 0 of nmax = 3
    spin, inc = EC.GRID_CASES['spin 0.94 / 60 deg']
    a70, b70 = EC.grid_rays()
    one, count1, status1 = host_program(a70, b70, spin, inc, 1, tag='nmax1')
    three, count3, status3 = host_program(a70, b70, spin, inc, 3, tag='nmax3')
    assert one.tobytes() == np.ascontiguousarray(three[:, :, :1]).tobytes() and np.array_equal(count1, np.minimum(count3, 1))
    assert (status1 <= status3).all() and (status1 < status3).any()


# ---- ray_geos and equatorial_ring

@pytest.fixture(scope='module')
def grid12():
    return G.image_plane_geos(0.94, INC60, EC.FOV, EC.FOV, ngeo=60, num_alpha=12, num_beta=12)


def test_ray_geos_on_a_grids_rays_is_the_grids_record(grid12):
    rays = G.ray_geos(0.94, INC60, grid12.alpha.ravel(), grid12.beta.ravel(), ngeo=60)
    assert list(rays) == list(grid12) and rays.dims == {'pix': 144, 'geo': 60} and kgeo.ray_geos is G.ray_geos
    for k in grid12:
        g, w = np.asarray(rays[k]), np.asarray(grid12[k])
        assert g.dtype == w.dtype and g.shape == ((144,) + w.shape[2:] if w.ndim else ()), k
        assert g.tobytes() == w.tobytes(), k


def _crossings_of(geos):
    alpha, beta = np.asarray(geos.alpha).ravel(), np.asarray(geos.beta).ravel()
    return G.equatorial_crossings(alpha, np.where(beta == 0.0, 1e-9, beta), geos.spin, geos.inc, nmax=2)


def _check_ring(geos, c, mbar, ring):
    mino = np.asarray(geos.mino).reshape(-1, geos.mino.shape[-1])
    ring = ring.reshape(mino.shape)
    has = c.count > mbar
    assert set(np.unique(ring)) <= {0.0, 1.0}
    assert np.array_equal(ring.sum(axis=1), has.astype(np.float64))               # exactly one 1.0 on a crossing ray, none elsewhere
    want = np.abs(mino[has] - c.mino[has, mbar][:, None]).argmin(axis=1)
    assert np.array_equal(ring[has].argmax(axis=1), want)
    return int(has.sum())


def test_equatorial_ring_marks_the_sample_nearest_the_crossing(grid12):
    c = _crossings_of(grid12)
    for mbar, least in ((0, 100), (1, 10)):
        ring = emission.equatorial_ring(grid12, mbar)
        assert ring.shape == grid12.mino.shape and ring.dtype == np.float64
        assert _check_ring(grid12, c, mbar, ring) >= least
    assert emission.equatorial_ring(grid12, 5).sum() == 0                          # no ray of this grid has a sixth crossing
    rays = G.ray_geos(0.94, INC60, [-8.0, -1.5, 0.5, 0.5, 2.75, 4.75, 7.0, 0.2, 3.0], [1.0, 4.0, 5.0, -5.0, 5.0, -4.0, -6.0, 0.1, 0.0], ngeo=50)
    assert rays.mino.shape == (9, 50) and rays.alpha.shape == (9,)
    c = _crossings_of(rays)
    for mbar, least in ((0, 7), (1, 4)):
        ring = emission.equatorial_ring(rays, mbar)
        assert ring.shape == (9, 50) and _check_ring(rays, c, mbar, ring) >= least


# ---- equatorial lensing on the host

def test_r_equatorial_returns_radius_and_mino_time_of_the_crossing():
    spin, inc = EC.GRID_CASES['spin 0.94 / 60 deg']
    alpha, beta = EC.grid_rays()
    cross, count, _, _ = EC.host_crossings(spin, inc)
    for mbar in (0, 1):
        out = kgeo.equatorial_lensing.r_equatorial(spin, np.inf, inc, mbar, alpha, beta)         # r_o = inf: distance 1000
        assert np.array_equal(out[0], cross[1][:, mbar], equal_nan=True) and np.array_equal(out[1], -cross[0][:, mbar], equal_nan=True)
    one = kgeo.equatorial_lensing.r_equatorial(spin, np.inf, inc, 0, float(alpha[3]), float(beta[3]))  # the reference's call: one ray
    assert one[0].shape == one[1].shape == (1,) and one[0][0] == cross[1][3, 0]


@pytest.mark.parametrize('mbar', [0, 1])
def test_rho_of_req_brackets_the_requested_radius(mbar):
    EL = kgeo.equatorial_lensing
    spin, req, kw = 0.94, 6.0, dict(distance=50.0, h=0.05)
    varphis = np.deg2rad([10.0, 100.0, 200.0, 300.0])
    rho, vp, alpha, beta = EL.rho_of_req(spin, INC60, req, mbar=mbar, varphis=varphis, **kw)
    assert np.array_equal(vp, varphis) and np.array_equal(alpha, rho * np.cos(varphis)) and np.array_equal(beta, rho * np.sin(varphis))
    inner = EL.r_equatorial(spin, 50.0, INC60, mbar, alpha * (1 - 1e-6), beta * (1 - 1e-6), h=0.05)[0]
    outer = EL.r_equatorial(spin, 50.0, INC60, mbar, alpha * (1 + 1e-6), beta * (1 + 1e-6), h=0.05)[0]
    print('\n[rho_of_req, host] mbar %d: rho %s, r_cross - req at rho (1 -+ 1e-6): %s / %s' % (mbar, rho, inner - req, outer - req))
    assert (inner < req).all() and (outer > req).all()
    with pytest.raises(ValueError, match='req must lie'):
        EL.rho_of_req(spin, INC60, 60.0, varphis=varphis, **kw)


# ---- back ends, arguments, library conventions

def test_unknown_backend_is_a_value_error(grid12):
    EL = kgeo.equatorial_lensing
    for call in (lambda: G.equatorial_crossings([3.0], [4.0], 0.6, 1.0, backend='bogus'),
                 lambda: G.ray_geos(0.6, 1.0, [3.0], [4.0], ngeo=4, backend='bogus'),
                 lambda: emission.equatorial_ring(grid12, 0, backend='bogus'),
                 lambda: EL.r_equatorial(0.6, np.inf, 1.0, 0, 3.0, 4.0, backend='bogus'),
                 lambda: EL.rho_of_req(0.6, 1.0, 6.0, varphis=[0.3], backend='bogus')):
        with pytest.raises(ValueError, match='bogus'):
            call()
    for inc in (0.5 * np.pi, 0.5 * np.pi - 5e-7, 0.0):
        with pytest.raises(ValueError, match='inclination must'):
            G.equatorial_crossings([3.0], [4.0], 0.6, inc)
    with pytest.raises(ValueError, match='nmax must'):
        G.equatorial_crossings([3.0], [4.0], 0.6, 1.0, nmax=0)


def test_hip_backend_needs_a_device_and_never_falls_back(grid12):
    import torch
    import __graft_entry__ as entry
    from bhnerf_amd import _hip
    entry.build()
    calls = (lambda: G.equatorial_crossings([3.0], [4.0], 0.6, 1.0, backend='hip'),
             lambda: G.ray_geos(0.6, 1.0, [3.0], [4.0], ngeo=4, backend='hip'),
             lambda: emission.equatorial_ring(grid12, 0, backend='hip'),
             lambda: kgeo.equatorial_lensing.r_equatorial(0.6, np.inf, 1.0, 0, 3.0, 4.0, backend='hip'))
    for call in calls:
        if torch.cuda.is_available():
            call()                                                      # a device is present: the call goes through
        else:
            with pytest.raises(_hip.HipError):
                call()


def test_argument_validation_returns_einval_before_any_device_call():
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.eql_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    good = dict(alpha=p, beta=p, n=4, spin=0.5, inclination=1.0, distance=1000.0, M=1.0, h=0.02, r_c=5.0, max_steps=1000, nmax=3,
                cross=p, count=p, status=p)
    order = list(good)
    bad = [(dict(alpha=None), b'null'), (dict(beta=None), b'null'), (dict(cross=None), b'null'), (dict(count=None), b'null'),
           (dict(status=None), b'null'), (dict(n=0), b'ray count'), (dict(n=-3), b'ray count'), (dict(nmax=0), b'nmax must'),
           (dict(nmax=-2), b'nmax must'), (dict(h=0.0), b'step h'), (dict(h=float('nan')), b'step h'), (dict(r_c=0.0), b'r_c must'),
           (dict(max_steps=0), b'max_steps must'), (dict(M=0.0), b'M must'), (dict(M=-1.0), b'M must'), (dict(spin=1.0001), b'|spin|'),
           (dict(spin=float('nan')), b'|spin|'), (dict(inclination=0.0), b'inclination must'), (dict(inclination=-0.3), b'inclination must'),
           (dict(inclination=0.5 * np.pi + 1e-9), b'inclination must'), (dict(inclination=float('nan')), b'inclination must'),
           (dict(inclination=0.5 * np.pi), b'sits in the plane'), (dict(inclination=0.5 * np.pi - 5e-7), b'sits in the plane')]
    for change, word in bad:
        a = dict(good, **change)
        rc = lib.bhn_eql_crossings(*[a[k] for k in order], None)
        assert rc == 1, (change, rc)                                # BHN_EINVAL
        msg = lib.bhn_eql_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_eql'):
            _hip.eql_check(rc)


def test_crossings_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_eql.so: the dynamic symbol table is the declarations of include/bhnerf_eql.h and nothing else, the ctypes table binds
    exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or ctypes
    table knows a name that begins with bhn_eql (side_lib_support.assert_library_conventions, for a fifth library)."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_eql.h'))))
    assert declared == sorted(_hip.EQL_SIGNATURES) == ['bhn_eql_crossings', 'bhn_eql_last_error']
    defined = side._symbols(_hip.EQL_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.EQL_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert len(side.LIBRARIES) == 4 and set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.LIBRARIES['libbhnerf_eql'] == (_hip.EQL_LIB_PATH, _hip.EQL_SIGNATURES, 'bhn_eql_last_error', None)
    for other_header, path, table in side.LIBRARIES:
        assert 'bhn_eql' not in side._header(other_header), other_header
        assert 'bhn_eql' not in side._symbols(getattr(_hip, path), '--defined-only'), path
        assert not any(k.startswith('bhn_eql') for k in getattr(_hip, table)), other_header
    # and the new library knows no other library's names
    for prefix in ('bhn_kerr', 'bhn_eht', 'bhn_grf'):
        assert prefix not in side._header('bhnerf_eql.h') and prefix not in defined, prefix
