"""CPU tests of the (g, J) library (libbhnerf_grf.so, csrc/gr_factors.hip; kgeo.emission_factors): everything about it that needs no
device.

The per-point arithmetic lives in csrc/gr_factors.h and compiles with a plain C++ compiler.  tools/gr_factors_host.cpp is a
stand-alone program around it that walks the library's launches workgroup by workgroup; here it is built with
g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process on the cases of tests/gr_factor_cases.py, and compared with the NumPy
functions of kgeo.py composed as alma.image_plane_model composes them -- the same arithmetic the device lanes run, so what is checked
is the restatement itself, and the sanitizers check the index arithmetic (the k -+ 1 neighbours at both ends of a ray, the tail
workgroup, the two reduction stages) on blocks of exactly the documented size.  Nothing is loaded into this Python process but the
library, for the argument checks.  Metric and bound: tests/gr_factor_cases.py (GR_TOL = 1e-10); the measured figures are printed.

Also here: kgeo.emission_factors(backend='numpy') is the composed functions bit for bit, back-end selection, BHN_EINVAL before any
device call, and the library's symbol table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gr_factor_cases as gc                                           # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import kgeo                                            # noqa: E402


_HOST = {}


def host_case(name, V_frac=0.0, spectral_index=1):
    """(record, reference) of a case on the NumPy tracer, computed once and left unchanged."""
    if name not in _HOST:
        _HOST[name] = gc.trace(name)
    key = (name, V_frac, spectral_index)
    if key not in _HOST:
        _HOST[key] = gc.reference(name, _HOST[name], V_frac, spectral_index)
    return _HOST[name], _HOST[key]


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/gr_factors_host.cpp built with the sanitizers -> a function of a record and the parameters -> (g, b, mean, J)."""
    exe, work = side.build_host_program(tmp_path_factory, 'gr_factors_host')

    def run(geos, Omega, field, domain, fill, V_frac, spectral_index, tag):
        shape = geos.r.shape
        ngeo, n = shape[-1], geos.r.size // shape[-1]
        S = 4 if V_frac != 0 else 3
        head = [n, ngeo, geos.spin, geos.M, geos.E, geos.inc, 0.0, float(fill), field[0], field[1], field[2], domain[0], domain[1], domain[2],
                1.0, gc.Q_FRAC, V_frac, spectral_index]
        parts = [np.asarray(head, dtype=np.float64)] + [np.asarray(geos[k], dtype=np.float64).ravel() for k in gc.POINT_FIELDS]
        parts += [np.asarray(Omega, dtype=np.float64).ravel()] + [np.asarray(geos[k], dtype=np.float64).ravel() for k in gc.RAY_FIELDS]
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        np.concatenate(parts).tofile(fin)
        side.run_host(exe, fin, fout)
        raw = np.fromfile(fout, dtype=np.float64)
        total = n * ngeo
        assert raw.size == total + 3 * total + 1 + S * total        # the documented sizes, nothing else
        return (raw[:total].reshape(shape), raw[total:4 * total].reshape(shape + (3,)), raw[4 * total],
                raw[4 * total + 1:].reshape((S,) + shape))
    return run


@pytest.mark.parametrize('name,V_frac,spectral_index', gc.VARIANTS)
def test_host_build_of_the_point_code_equals_the_numpy_functions(host_program, name, V_frac, spectral_index):
    geos, ref = host_case(name, V_frac, spectral_index)
    gc.assert_conditions(name, ref)
    tag = 'c%s_%d' % (name, int(V_frac != 0))
    g, b, mean, J = host_program(geos, ref['Omega'], gc.CASES[name][3], gc.domain_of(name), True, V_frac, spectral_index, tag)
    g_nan = host_program(geos, ref['Omega'], gc.CASES[name][3], gc.domain_of(name), False, V_frac, spectral_index, tag + 'n')[0]
    errs = gc.errors(g, b, mean, J, ref, got_g_nan=g_nan)
    gc.report('host build', name, V_frac, spectral_index, errs)
    print('    %d points, %d in the domain, %d NaN in g before the fill, smallest timelike margin %.1e'
          % (geos.r.size, ref['domain'].sum(), np.isnan(ref['g_nan']).sum(), np.nanmin(ref['margin'])))
    assert max(errs.values()) <= gc.GR_TOL, (name, {k: e for k, e in errs.items() if e > gc.GR_TOL})


@pytest.mark.parametrize('name,V_frac,spectral_index', [('A', 0.0, 1), ('C', 0.0, 1), ('E', 0.0, 1), ('B', 0.01, 1.5)])
def test_numpy_backend_is_the_composed_functions_bit_for_bit(name, V_frac, spectral_index):
    geos, ref = host_case(name, V_frac, spectral_index)
    arad, avert, ator = gc.CASES[name][3]
    consts = dict(arad=arad, avert=avert, ator=ator)
    with np.errstate(all='ignore'):
        g, J = kgeo.emission_factors(geos, ref['Omega'], consts, gc.domain_of(name), Q_frac=gc.Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)
        g2, J2 = kgeo.emission_factors(geos, ref['Omega'], consts, gc.domain_of(name), Q_frac=gc.Q_FRAC, V_frac=V_frac,
                                       spectral_index=spectral_index, backend='numpy')
        g_nan, none = kgeo.emission_factors(geos, ref['Omega'], fillna=False)
    assert none is None
    assert np.array_equal(g, ref['g']) and np.array_equal(g2, ref['g']) and np.array_equal(g_nan, ref['g_nan'], equal_nan=True)
    assert J.shape == ref['J'].shape == ((4 if V_frac else 3),) + geos.r.shape
    assert np.array_equal(J, ref['J'], equal_nan=True) and np.array_equal(J2, ref['J'], equal_nan=True)
    # without a domain the field is taken as it is
    with np.errstate(all='ignore'):
        J_raw = kgeo.emission_factors(geos, ref['Omega'], consts, None, Q_frac=gc.Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)[1]
        umu = kgeo.azimuthal_velocity_vector(geos, ref['Omega'])
        want = kgeo.parallel_transport(geos, umu, ref['g'], ref['b'], Q_frac=gc.Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)
    assert np.array_equal(J_raw, want, equal_nan=True)


def test_image_plane_model_default_is_unchanged_and_names_are_checked():
    """alma.image_plane_model without 'factors' and with 'numpy' give the same bytes: those of the functions it composed before
    kgeo.emission_factors existed, composed here in the same way (the domain from the record's z)."""
    from bhnerf_amd import alma, constants, emission
    params = dict(fov_M=18.0, z_width=4, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0, avert=1, ator=0), Omega_dir='ccw',
                  num_alpha=3, num_beta=2, t_start_obs=9.3)
    geos, Omega, J = alma.image_plane_model(np.deg2rad(60.0), 0.5, params)
    geos2, Omega2, J2 = alma.image_plane_model(np.deg2rad(60.0), 0.5, dict(params, factors='numpy'))
    assert np.array_equal(Omega, Omega2) and J.tobytes() == J2.tobytes() and J.shape == (3, 3, 2, 100)
    umu = kgeo.azimuthal_velocity_vector(geos, Omega)
    g = kgeo.doppler_factor(geos, umu)
    b = kgeo.magnetic_field_fluid_frame(geos, umu, **params['b_consts'])
    domain = (np.abs(geos.z) < 4) & (geos.r > float(constants.isco_pro(0.5))) & (geos.r < 9.0)
    assert domain.sum() >= 10
    b = b / np.sqrt((b[domain] ** 2).sum(axis=-1)).mean()
    with np.errstate(all='ignore'):
        want = kgeo.parallel_transport(geos, umu, g, b, Q_frac=0.85, V_frac=0)
    assert np.abs(np.nan_to_num(want)).max() > 0.0
    assert J.tobytes() == emission.rotate_evpa(np.nan_to_num(want, nan=0.0), 0.0).tobytes()
    with pytest.raises(ValueError, match='bogus'):
        alma.image_plane_model(np.deg2rad(60.0), 0.5, dict(params, factors='bogus'))


def test_unknown_backend_is_a_value_error():
    from bhnerf_amd import network
    geos, ref = host_case('tiny')
    with pytest.raises(ValueError, match='bogus'):
        kgeo.emission_factors(geos, ref['Omega'], backend='bogus')
    with pytest.raises(ValueError, match='bogus'):
        network.raytracing_args(geos, ref['Omega'], -100.0, 0.0, backend='bogus')


def test_a_single_sample_per_ray_is_numpys_value_error_on_both_backends():
    geos, ref = host_case('tiny')
    one = type(geos)({k: (np.asarray(v)[..., :1] if np.ndim(v) == 3 else v) for k, v in geos.items()})
    for backend in ('numpy', 'hip'):
        with pytest.raises(ValueError, match='too small to calculate a numerical gradient'):
            kgeo.emission_factors(one, ref['Omega'][..., :1], backend=backend)


def test_hip_backend_without_a_device_raises_the_package_error():
    import torch
    from bhnerf_amd import _hip, alma, network
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import __graft_entry__ as entry
    entry.build()
    geos, ref = host_case('tiny')
    with pytest.raises(_hip.HipError):
        kgeo.emission_factors(geos, ref['Omega'], backend='hip')
    with pytest.raises(_hip.HipError):
        kgeo.emission_factors(geos, ref['Omega'], dict(arad=0, avert=1, ator=0), gc.domain_of('tiny'), backend='hip')
    with pytest.raises(_hip.HipError):
        network.raytracing_args(geos, ref['Omega'], -100.0, 0.0, backend='hip')
    params = dict(fov_M=40.0, z_width=4, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0, avert=1, ator=0), Omega_dir='cw',
                  num_alpha=2, num_beta=2, t_start_obs=9.3, factors='hip')
    with pytest.raises(_hip.HipError):                              # params['factors'] reaches the library
        alma.image_plane_model(np.deg2rad(12.0), 0.0, params)


def test_argument_validation_returns_einval_before_any_device_call():
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.grf_lib()
    p = 4096                                # never dereferenced: every call below is refused before a launch
    P = C.c_void_p(p)
    fields = gc.POINT_FIELDS + gc.RAY_FIELDS

    def record(**change):
        kw = dict(n=4, ngeo=8, spin=0.5, M=1.0, E=1.0, inc=1.0, **{k: p for k in fields})
        kw.update(change)
        return _hip.bhn_grf_geos(kw['n'], kw['ngeo'], *[kw[k] for k in fields], kw['spin'], kw['M'], kw['E'], kw['inc'])

    calls = {
        'doppler': lambda rec, a: lib.bhn_grf_doppler(rec, a.get('Omega', P), 0.0, 1, a.get('g', P), None),
        'fluid_field': lambda rec, a: lib.bhn_grf_fluid_field(rec, a.get('Omega', P), 0.0, 1.0, 0.0, a.get('b', P), None),
        'domain_mean': lambda rec, a: lib.bhn_grf_domain_mean(rec, a.get('b', P), 4.0, 2.0, 9.0, a.get('mean', P), a.get('ws', P),
                                                               a.get('ws_bytes', 1 << 20), None),
        'transport': lambda rec, a: lib.bhn_grf_transport(rec, a.get('Omega', P), a.get('g', P), a.get('b', P), a.get('divisor', None),
                                                           a.get('Q_frac', 0.5), 0.0, 1.0, a.get('J', P), None),
    }
    bad_records = [(None, b'null geos')] + [(record(**{k: None}), b'null field') for k in fields] + [
        (record(n=0), b'ray count'), (record(n=-2), b'ray count'), (record(ngeo=1), b'ngeo must'), (record(ngeo=0), b'ngeo must'),
        (record(ngeo=-4), b'ngeo must'), (record(n=1 << 45, ngeo=1 << 20), b'too many points')]
    bad_args = {
        'doppler': [(dict(Omega=None), b'null Omega'), (dict(g=None), b'null output')],
        'fluid_field': [(dict(Omega=None), b'null Omega'), (dict(b=None), b'null output')],
        'domain_mean': [(dict(b=None), b'null b or mean'), (dict(mean=None), b'null b or mean'), (dict(ws=None), b'workspace'),
                        (dict(ws=C.c_void_p(p + 4)), b'misaligned')],
        'transport': [(dict(Omega=None), b'null Omega'), (dict(g=None), b'null g, b or J'), (dict(b=None), b'null g, b or J'),
                      (dict(J=None), b'null g, b or J'), (dict(Q_frac=1.5), b'Q_frac'), (dict(Q_frac=-0.1), b'Q_frac')],
    }
    for name, call in calls.items():
        cases = [(C.byref(rec) if rec is not None else None, {}, word) for rec, word in bad_records]
        cases += [(C.byref(record()), change, word) for change, word in bad_args[name]]
        for rec, change, word in cases:
            rc = call(rec, change)
            assert rc == _hip.BHN_EINVAL, (name, change, word, rc)
            msg = lib.bhn_grf_last_error()
            assert msg and word in msg, (name, change, msg)
            with pytest.raises(_hip.HipError, match='libbhnerf_grf'):
                _hip.grf_check(rc)
    # a workspace that is too small has a code of its own, also before any launch
    rc = calls['domain_mean'](C.byref(record()), dict(ws_bytes=8))
    assert rc == _hip.BHN_EWORKSPACE and b'needed' in lib.bhn_grf_last_error()
    assert lib.bhn_grf_ws_bytes(4, 8) == 16 and lib.bhn_grf_ws_bytes(70, 40) == 11 * 16 and lib.bhn_grf_ws_bytes(64, 4) == 16
    assert lib.bhn_grf_ws_bytes(0, 8) == 0 and lib.bhn_grf_ws_bytes(4, 1) == 0 and lib.bhn_grf_ws_bytes(1 << 45, 1 << 20) == 0


def test_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_grf.so: the dynamic symbol table is the declarations of include/bhnerf_grf.h and nothing else, the ctypes table
    binds exactly those, and the library references no allocator, no getenv and no synchronisation.  The other three libraries,
    their headers and their ctypes tables do not know the new names."""
    from bhnerf_amd import _hip
    side.assert_library_conventions('bhnerf_grf.h', _hip.GRF_LIB_PATH, _hip.GRF_SIGNATURES, 'bhn_grf',
                                    ['bhn_grf_domain_mean', 'bhn_grf_doppler', 'bhn_grf_fluid_field', 'bhn_grf_last_error',
                                     'bhn_grf_transport', 'bhn_grf_ws_bytes'])
