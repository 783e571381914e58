"""CPU tests of the GPU Kerr tracer (bhn_kerr_trace, csrc/kerr_trace.hip): everything about it that needs no device.

The per-ray stepping code lives in csrc/kerr_trace.h and compiles with a plain C++ compiler.  tools/kerr_trace_host.cpp is a
stand-alone program around it; here it is built with g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process on small ray
sets, and compared with geodesics._integrate (the NumPy tracer) -- the same arithmetic the device lanes run, so what is checked is
the restatement itself (scheme, step rule, constants, capture / escape rules, the Hermite sampling and the end-state fill), and the
sanitizers check the sample-index arithmetic (several targets inside one step, the fill that starts at the next unwritten sample)
on output blocks of exactly the documented size.  Nothing is loaded into this Python process.

Bound: each of the seven rows (mino, r, theta, phi, t, vr, vth), relative to the row's largest magnitude over the grid, within
GR_TOL = 1e-10 (tests/test_geodesics_cpu.py).  Rounding-size noise on every right-hand-side evaluation moves these grids by
<= 5e-12, a one-ulp change of (alpha, beta) by <= 8e-13; the restatement differs from NumPy by the maths library's sin / cos,
s * s * s for s ** 3 and cos / sin for 1 / tan only.  The measured maxima are printed.

Also here: back-end selection of geodesics.trace / image_plane_geos, and bhn_kerr_trace's argument validation (BHN_EINVAL with a
message before any device call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import geodesics as G                                  # noqa: E402

GR_TOL = 1e-10
ROWS = ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth')
H, R_C, MAX_STEPS = 0.02, 5.0, 400000

# name -> (spin, inclination, alpha_range, beta_range, num_alpha, num_beta, ngeo, distance, M)
CASES = {
    'spin 0.94 / 60 deg, 8x6': (0.94, np.deg2rad(60.0), (-9.0, 9.0), (-9.0, 9.0), 8, 6, 40, 1000.0, 1.0),
    'spin 0.94 / 17 deg, 8x6': (0.94, np.deg2rad(17.0), (-9.0, 9.0), (-9.0, 9.0), 8, 6, 40, 1000.0, 1.0),
    'flat space, 2x2': (0.0, np.deg2rad(50.0), (2.0, 6.0), (-5.0, -3.0), 2, 2, 30, 200.0, 1e-9),
    'spin 0.94 / 60 deg, 8x6, ngeo 1': (0.94, np.deg2rad(60.0), (-9.0, 9.0), (-9.0, 9.0), 8, 6, 1, 1000.0, 1.0),
    'one captured ray': (0.94, np.deg2rad(60.0), (0.5, 0.5), (0.25, 0.25), 1, 1, 40, 1000.0, 1.0),
    'one scattered ray': (0.94, np.deg2rad(60.0), (-7.0, -7.0), (3.0, 3.0), 1, 1, 40, 1000.0, 1.0),
}
CAPTURES = {'spin 0.94 / 60 deg, 8x6': 6, 'spin 0.94 / 17 deg, 8x6': 6, 'flat space, 2x2': 0, 'spin 0.94 / 60 deg, 8x6, ngeo 1': 6,
            'one captured ray': 1, 'one scattered ray': 0}          # at least this many rays end at the horizon


def rays(case):
    spin, inc, ar, br, na, nb, ngeo, dist, M = CASES[case]
    alpha, beta = np.meshgrid(np.linspace(*ar, na), np.linspace(*br, nb), indexing='ij')
    beta = np.where(beta == 0.0, 1e-9, beta)
    return alpha.ravel(), beta.ravel()


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/kerr_trace_host.cpp built with the sanitizers -> a function (case) -> (end (7, n), status (n), samples (7, n, ngeo))."""
    exe, work = side.build_host_program(tmp_path_factory, 'kerr_trace_host')

    def run(alpha, beta, spin, inc, dist, M, ngeo, max_steps=MAX_STEPS, tag='case'):
        n = alpha.size
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        np.concatenate([[n, ngeo, max_steps, spin, inc, dist, M, H, R_C], alpha, beta]).astype(np.float64).tofile(fin)
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        assert len(raw) == 8 * 7 * n + 4 * n + 8 * 7 * n * ngeo     # the documented sizes, nothing else
        end = np.frombuffer(raw, dtype=np.float64, count=7 * n).reshape(7, n)
        status = np.frombuffer(raw, dtype=np.int32, count=n, offset=8 * 7 * n)
        samples = np.frombuffer(raw, dtype=np.float64, count=7 * n * ngeo, offset=8 * 7 * n + 4 * n).reshape(7, n, ngeo)
        return end, status, samples
    return run


_NUMPY = {}


def numpy_trace(case):
    """(end (7, n), samples (7, n, ngeo)) of geodesics._integrate, computed once per case and left unchanged."""
    if case not in _NUMPY:
        spin, inc, ar, br, na, nb, ngeo, dist, M = CASES[case]
        alpha, beta = rays(case)
        mino_end, y_end, _, _ = G._integrate(alpha, beta, spin, inc, dist, M, H, R_C, MAX_STEPS)
        target = (np.arange(1, ngeo + 1)[None, :] / float(ngeo)) * mino_end[:, None]
        samp, _, _ = G._integrate(alpha, beta, spin, inc, dist, M, H, R_C, MAX_STEPS, targets=target)
        _NUMPY[case] = (np.concatenate([mino_end[None], y_end]), samp)
    return _NUMPY[case]


def row_errors(got, want):
    """Per row: max |got - want| over the grid / the row's largest magnitude."""
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    ax = tuple(range(1, want.ndim))
    return np.abs(got - want).max(axis=ax) / np.maximum(np.abs(want).max(axis=ax), 1e-300)


@pytest.mark.parametrize('case', list(CASES))
def test_host_build_of_the_stepping_code_equals_the_numpy_tracer(host_program, case):
    spin, inc, ar, br, na, nb, ngeo, dist, M = CASES[case]
    alpha, beta = rays(case)
    end, status, samples = host_program(alpha, beta, spin, inc, dist, M, ngeo, tag='c%d' % list(CASES).index(case))
    want_end, want_samples = numpy_trace(case)
    assert (status > 0).all() and (status < MAX_STEPS).all()         # every element written (0x7F7F7F7F where not), every ray finished
    r_hor = M + np.sqrt(max(M * M - (spin * M) ** 2, 0.0))
    captured = want_end[1] < 1.2 * r_hor
    assert captured.sum() >= CAPTURES[case] and ((want_end[1] > dist) | captured).all()
    e_end, e_smp = row_errors(end, want_end), row_errors(samples, want_samples)
    print('\n[kerr trace, host build] %-34s %d rays (%d captured), steps %d..%d' % (case, alpha.size, captured.sum(), status.min(), status.max()))
    print('    end states ' + '  '.join('%s %.1e' % (k, e) for k, e in zip(ROWS, e_end)))
    print('    samples    ' + '  '.join('%s %.1e' % (k, e) for k, e in zip(ROWS, e_smp)))
    assert e_end.max() <= GR_TOL and e_smp.max() <= GR_TOL, (case, e_end, e_smp)
    assert np.array_equal(samples[0, :, -1], end[0])                 # the last target is the ray's total Mino time


def test_an_exhausted_step_budget_is_reported_not_looped(host_program):
    """max_steps = 10: status -1 for every ray, and every element of end and samples still written (the state reached)."""
    spin, inc = 0.94, np.deg2rad(60.0)
    alpha, beta = np.array([-7.0, 0.5, 3.0, 8.0]), np.array([3.0, 0.25, -4.0, 1.0])
    end, status, samples = host_program(alpha, beta, spin, inc, 1000.0, 1.0, 5, max_steps=10, tag='budget')
    assert (status == -1).all()
    assert np.isfinite(end).all() and np.isfinite(samples).all()
    assert (end[1] < 1000.0).all() and (end[1] > 900.0).all() and (end[0] > 0).all()         # ten steps inwards from the observer
    assert np.array_equal(samples, np.repeat(end[:, :, None], 5, axis=2))
    # ngeo = 0: end states only, no sample block at all
    end0, status0, samples0 = host_program(alpha, beta, spin, inc, 1000.0, 1.0, 0, tag='ngeo0')
    assert samples0.size == 0 and (status0 > 0).all()
    want = G.trace(alpha, beta, spin, inc)
    assert row_errors(end0, np.concatenate([want[0][None], want[1]])).max() <= GR_TOL


def test_default_backend_is_the_numpy_tracer_bit_for_bit():
    args = (0.6, np.deg2rad(60.0), (-7.0, 7.0), (-7.0, 7.0))
    kw = dict(ngeo=12, num_alpha=3, num_beta=2)
    a, b = G.image_plane_geos(*args, **kw), G.image_plane_geos(*args, backend='numpy', **kw)
    assert list(a) == list(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    ta, tb = G.trace([3.0, -6.0], [4.0, 1.0], 0.6, 1.0), G.trace([3.0, -6.0], [4.0, 1.0], 0.6, 1.0, backend='numpy')
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb))


def test_unknown_backend_is_a_value_error():
    with pytest.raises(ValueError, match='bogus'):
        G.image_plane_geos(0.6, 1.0, (-7.0, 7.0), (-7.0, 7.0), ngeo=4, num_alpha=2, num_beta=2, backend='bogus')
    with pytest.raises(ValueError, match='bogus'):
        G.trace([3.0], [4.0], 0.6, 1.0, backend='bogus')


def test_hip_backend_without_a_device_raises_the_package_error():
    import torch
    from bhnerf_amd import _hip, alma
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import __graft_entry__ as entry
    entry.build()
    with pytest.raises(_hip.HipError):
        G.image_plane_geos(0.6, 1.0, (-7.0, 7.0), (-7.0, 7.0), ngeo=4, num_alpha=2, num_beta=2, backend='hip')
    with pytest.raises(_hip.HipError):
        G.trace([3.0], [4.0], 0.6, 1.0, backend='hip')
    params = dict(fov_M=40.0, z_width=4, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0, avert=1, ator=0), Omega_dir='cw',
                  num_alpha=2, num_beta=2, t_start_obs=9.3, tracer='hip')
    with pytest.raises(_hip.HipError):                              # params['tracer'] reaches the tracer
        alma.image_plane_model(np.deg2rad(12.0), 0.0, params)
    with pytest.raises(ValueError, match='bogus'):
        alma.image_plane_model(np.deg2rad(12.0), 0.0, dict(params, tracer='bogus'))


def test_argument_validation_returns_einval_before_any_device_call():
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.kerr_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    good = dict(alpha=p, beta=p, n=4, spin=0.5, inclination=1.0, distance=1000.0, M=1.0, h=0.02, r_c=5.0, max_steps=1000, ngeo=8,
                samples=p, end=p, status=p)
    order = list(good)
    bad = [(dict(alpha=None), b'null'), (dict(beta=None), b'null'), (dict(end=None), b'null'), (dict(status=None), b'null'),
           (dict(n=0), b'ray count'), (dict(n=-3), b'ray count'), (dict(ngeo=-1), b'ngeo must'), (dict(samples=None), b'samples is NULL'),
           (dict(h=0.0), b'step h'), (dict(h=-0.02), b'step h'), (dict(h=float('nan')), b'step h'), (dict(r_c=0.0), b'r_c must'),
           (dict(r_c=-5.0), b'r_c must'), (dict(max_steps=0), b'max_steps must'), (dict(M=0.0), b'M must'), (dict(M=-1.0), b'M must'),
           (dict(spin=1.0001), b'|spin|'), (dict(spin=-1.5), b'|spin|'), (dict(spin=float('nan')), b'|spin|'),
           (dict(inclination=0.0), b'inclination must'), (dict(inclination=-0.3), b'inclination must'),
           (dict(inclination=0.5 * np.pi + 1e-9), b'inclination must'), (dict(inclination=float('nan')), b'inclination must')]
    for change, word in bad:
        a = dict(good, **change)
        rc = lib.bhn_kerr_trace(*[a[k] for k in order], None)
        assert rc == 1, (change, rc)                                # BHN_EINVAL
        msg = lib.bhn_kerr_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_kerr'):
            _hip.kerr_check(rc)


def test_tracer_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_kerr.so: the dynamic symbol table is the declarations of include/bhnerf_kerr.h and nothing else, the ctypes table
    binds exactly those, and the library references no allocator, no getenv and no synchronisation (the conventions of
    include/bhnerf_hip.h, which tests/test_abi_cpu.py holds libbhnerf_hip.so to).  The hot path's ABI is not touched: the tracer is
    not declared in include/bhnerf_hip.h and not exported by libbhnerf_hip.so."""
    from bhnerf_amd import _hip
    side.assert_library_conventions('bhnerf_kerr.h', _hip.KERR_LIB_PATH, _hip.KERR_SIGNATURES, 'bhn_kerr',
                                    ['bhn_kerr_last_error', 'bhn_kerr_trace'])
