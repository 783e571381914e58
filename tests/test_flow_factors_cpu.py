"""CPU tests of the general-flow (g, J) library (libbhnerf_flow.so, csrc/flow_factors.hip; kgeo.emission_factors with flow=): everything
about it that needs no device.

The per-point arithmetic lives in csrc/flow_factors.h (on csrc/gr_factors.h) and compiles with a plain C++ compiler.
tools/flow_factors_host.cpp is a stand-alone program around it that walks the library's launches workgroup by workgroup; here it is
built with g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process on the cases of tests/flow_factor_cases.py
and compared with the NumPy functions of kgeo.py composed directly -- the same arithmetic the device lanes run, on blocks of exactly the
documented size.  Nothing is loaded into this Python process but the library, for the argument checks.  Metric and bound:
tests/gr_factor_cases.py (GR_TOL = 1e-10); the measured figures are printed.  MEASURED (host build): umu, g and b equal NumPy's bit for bit
on every case; the largest figure of J over all cases, variants and both frames is 8.1e-13 (U of Z3, the fluid tetrad).

Also here: kgeo.emission_factors(backend='numpy', flow=...) is the hand-composed functions bit for bit, flow=None returns today's
bytes, the Keplerian umu through the array path against gr_factor_cases' reference, keyword and argument errors, and the library's
symbol table."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_factor_cases as fc                                         # noqa: E402
import gr_factor_cases as gc                                           # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import kgeo                                            # noqa: E402

POINT_FIELDS = gc.POINT_FIELDS + ('omega',)
_HOST = {}


def host_case(name, V_frac=0.0, spectral_index=1):
    """(record, reference) of a case on the NumPy tracer, computed once and left unchanged.  The V variant divides the field by its
    domain mean, the others take it as it is."""
    record = fc.CASES[name][0]
    if record not in _HOST:
        _HOST[record] = gc.trace(record)
    key = (name, V_frac, spectral_index)
    if key not in _HOST:
        divisor = None
        if V_frac != 0:
            divisor = fc.domain_mean(host_case(name)[1])
        _HOST[key] = fc.reference(name, _HOST[record], V_frac, spectral_index, divisor)
    return _HOST[record], _HOST[key]


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/flow_factors_host.cpp built with the sanitizers -> a function of a record and the parameters -> dict(umu, g, b, J)."""
    exe, work = side.build_host_program(tmp_path_factory, 'flow_factors_host')

    def run(geos, flow, field, fill, V_frac, spectral_index, zamo_frame, divisor, tag):
        shape = geos.r.shape
        ngeo, n = shape[-1], geos.r.size // shape[-1]
        total = n * ngeo
        given_umu = not isinstance(flow, tuple)
        beta, chi = (0.0, 0.0) if given_umu else flow[1:]
        given_b = not isinstance(field, dict)
        arad, avert, ator = (0.0, 0.0, 0.0) if given_b else (field['arad'], field['avert'], field['ator'])
        head = [n, ngeo, geos.spin, geos.M, geos.E, geos.inc, 0.0, float(fill), float(given_umu), beta, chi, float(given_b), arad, avert, ator,
                0.0 if divisor is None else divisor, fc.Q_FRAC, V_frac, spectral_index, float(zamo_frame)]
        parts = [np.asarray(head, dtype=np.float64)] + [np.asarray(geos[k], dtype=np.float64).ravel() for k in POINT_FIELDS]
        parts += [np.asarray(geos[k], dtype=np.float64).ravel() for k in gc.RAY_FIELDS]
        if given_umu:
            parts.append(np.asarray(flow, dtype=np.float64).ravel())
        if given_b:
            parts.append(np.asarray(field, dtype=np.float64).ravel())
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        np.concatenate(parts).tofile(fin)
        side.run_host(exe, fin, fout)
        raw = np.fromfile(fout, dtype=np.float64)
        S = 4 if (V_frac != 0 and not zamo_frame) else 3
        sizes = [('umu', 0 if given_umu else 4 * total, shape + (4,)), ('g', total, shape), ('b', 0 if given_b else 3 * total, shape + (3,)),
                 ('J', S * total, (S,) + shape)]
        assert raw.size == sum(size for _, size, _ in sizes)          # the documented sizes, nothing else
        out, at = {}, 0
        for key, size, shp in sizes:
            out[key] = raw[at:at + size].reshape(shp) if size else None
            at += size
        return out
    return run


def _field_for_library(name, ref):
    """What the library takes of the case's field: dict(arad, avert, ator), or the array of magnetic_field_spherical."""
    return fc.b_consts_of(name) if fc.CASES[name][3] == 'fluid' else ref['b']


@pytest.mark.parametrize('name,V_frac,spectral_index', fc.VARIANTS)
def test_host_build_of_the_point_code_equals_the_numpy_functions(host_program, name, V_frac, spectral_index):
    geos, ref = host_case(name, V_frac, spectral_index)
    fc.assert_conditions(name, geos, ref)
    field, tag = _field_for_library(name, ref), '%s_%d' % (name, int(V_frac != 0))
    out = host_program(geos, ref['flow'], field, True, V_frac, spectral_index, False, ref['divisor'], tag)
    g_nan = host_program(geos, ref['flow'], field, False, V_frac, spectral_index, False, ref['divisor'], tag + 'n')['g']
    assert (out['umu'] is not None) == (name in fc.SCALAR) and (out['b'] is not None) == isinstance(field, dict)
    J_zamo = None
    if name in fc.SCALAR:
        J_zamo = host_program(geos, ref['flow'], field, True, V_frac, spectral_index, True, ref['divisor'], tag + 'z')['J']
    errs = fc.errors(ref, umu=out['umu'], g=out['g'], g_nan=g_nan, b=out['b'], J=out['J'], J_zamo=J_zamo)
    fc.report('host build', name, V_frac, spectral_index, errs)
    print('    %d points, %d in the domain, %d NaN in g before the fill, smallest Delta %.1e'
          % (geos.r.size, ref['domain'].sum(), np.isnan(ref['g_nan']).sum(), np.asarray(geos.Delta).min()))
    assert max(errs.values()) <= fc.GR_TOL, (name, {k: e for k, e in errs.items() if e > fc.GR_TOL})


@pytest.mark.parametrize('name,V_frac,spectral_index', [('Z1', 0.01, 1.5), ('Z3', 0.0, 1), ('Za', 0.0, 1), ('Zs', 0.0, 1)])
def test_numpy_backend_with_a_flow_is_the_composed_functions_bit_for_bit(name, V_frac, spectral_index):
    geos, ref = host_case(name)
    record, beta, chi, kind, field = fc.CASES[name]
    kw = dict(Q_frac=fc.Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)
    flow, umu = ref['flow'], ref['umu']
    sel = ref['domain']
    with np.errstate(all='ignore'):
        fields = {'fluid': (dict(arad=0.3, avert=0.5, ator=0.8), kgeo.magnetic_field_fluid_frame(geos, umu, 0.3, 0.5, 0.8)),
                  'spherical': (dict(b_r=0.87, b_th=0.0, b_ph=0.5), kgeo.magnetic_field_spherical(geos, 0.87, 0.0, 0.5))}
        fields['array'] = (fields['fluid'][1] + 0.25 * fields['spherical'][1],) * 2
        g_only, none = kgeo.emission_factors(geos, flow=flow, fillna=False)
        assert none is None and np.array_equal(g_only, ref['g_nan'], equal_nan=True)
        for b_kind, (b_consts, b) in fields.items():
            for domain in (None, fc.domain_of(name)):
                bd = b if domain is None else b / np.sqrt((b[sel] ** 2).sum(axis=-1)).mean()
                want = kgeo.parallel_transport(geos, umu, ref['g'], bd, **kw)
                g, J = kgeo.emission_factors(geos, None, b_consts, domain, flow=flow, backend='numpy', **kw)
                assert np.array_equal(g, ref['g']), (b_kind, domain)
                assert J.shape == ((4 if V_frac else 3),) + geos.r.shape and np.array_equal(J, want, equal_nan=True), (b_kind, domain)
                if name in fc.SCALAR:
                    want = kgeo.parallel_transport_zamo(geos, beta, chi, ref['g'], bd, Q_frac=fc.Q_FRAC, spectral_index=spectral_index)
                    g, J = kgeo.emission_factors(geos, None, b_consts, domain, flow=flow, frame='zamo', **kw)
                    assert np.array_equal(g, ref['g']) and J.shape == (3,) + geos.r.shape and np.array_equal(J, want, equal_nan=True), (b_kind, domain)
        if name not in fc.SCALAR:                                       # per-point beta and chi are evaluated on the host
            g, J = kgeo.emission_factors(geos, flow=('zamo',) + fc.per_point(name, geos), b_consts=fields['spherical'][0], **kw)
            want = kgeo.parallel_transport(geos, umu, ref['g'], fields['spherical'][1], **kw)
            assert np.array_equal(g, ref['g']) and np.array_equal(J, want, equal_nan=True)


@pytest.mark.parametrize('name', ['A', 'B'])
def test_without_a_flow_the_bytes_are_todays(name):
    if name not in _HOST:
        _HOST[name] = gc.trace(name)
    geos = _HOST[name]
    ref = gc.reference(name, geos)
    consts = dict(zip(('arad', 'avert', 'ator'), gc.CASES[name][3]))
    with np.errstate(all='ignore'):
        g, J = kgeo.emission_factors(geos, ref['Omega'], consts, gc.domain_of(name), Q_frac=gc.Q_FRAC, V_frac=0.0)
        g2, J2 = kgeo.emission_factors(geos, Omega=ref['Omega'], b_consts=consts, domain=gc.domain_of(name), Q_frac=gc.Q_FRAC, V_frac=0.0, flow=None,
                                       frame='fluid')
    assert g.tobytes() == g2.tobytes() == ref['g'].tobytes() and J.tobytes() == J2.tobytes() == ref['J'].tobytes()


def test_the_keplerian_umu_through_the_array_path_equals_the_azimuthal_reference(host_program):
    geos, ref = host_case('Zk')
    want = gc.reference('A', geos)
    gc.assert_conditions('A', want)
    with np.errstate(all='ignore'):
        g, J = kgeo.emission_factors(geos, flow=ref['umu'], b_consts=fc.b_consts_of('Zk'), domain=gc.domain_of('A'), Q_frac=gc.Q_FRAC, V_frac=0.0)
    assert np.array_equal(g, want['g']) and np.array_equal(J, want['J'], equal_nan=True)       # the same NumPy calls
    out = host_program(geos, ref['umu'], fc.b_consts_of('Zk'), True, 0.0, 1, False, want['mean'], 'Zk_mean')
    errs = gc.errors(out['g'], out['b'], want['mean'], out['J'], want)
    bitwise = {k: bool(np.array_equal(got, want[k], equal_nan=True)) for k, got in (('g', out['g']), ('b', out['b']), ('J', out['J']))}
    gc.report('flow host build, Keplerian umu', 'A', 0.0, 1, errs)
    print('    bitwise equal to the NumPy reference: %s' % bitwise)
    assert max(errs.values()) <= gc.GR_TOL, errs


def test_keyword_errors():
    geos, ref = host_case('Zt')
    flow, Omega = ref['flow'], np.zeros(geos.r.shape)
    with pytest.raises(ValueError, match='both'):
        kgeo.emission_factors(geos, Omega, flow=flow)
    with pytest.raises(ValueError, match='neither'):
        kgeo.emission_factors(geos)
    for backend in ('numpy', 'hip'):
        with pytest.raises(ValueError, match='frame'):
            kgeo.emission_factors(geos, flow=flow, frame='lab', backend=backend)
        with pytest.raises(ValueError, match="frame='zamo' needs a scalar ZAMO flow"):
            kgeo.emission_factors(geos, flow=ref['umu'], frame='zamo', backend=backend)
        with pytest.raises(ValueError, match="frame='zamo' needs a scalar ZAMO flow"):
            kgeo.emission_factors(geos, flow=('zamo', np.full(geos.r.shape, 0.5), 0.1), frame='zamo', backend=backend)
        with pytest.raises(ValueError, match="needs a scalar ZAMO flow"):
            kgeo.emission_factors(geos, Omega, frame='zamo', backend=backend)
        with pytest.raises(ValueError, match='umu array of shape'):
            kgeo.emission_factors(geos, flow=ref['umu'][..., :3], backend=backend)
        with pytest.raises(ValueError, match='kepler'):
            kgeo.emission_factors(geos, flow=('kepler', 0.5, 0.1), backend=backend)
        with pytest.raises(ValueError, match='b_consts must have the keys'):
            kgeo.emission_factors(geos, flow=flow, b_consts=dict(arad=1.0, b_th=0.0, b_ph=0.0), backend=backend)
        with pytest.raises(AttributeError, match='Q_frac'):
            kgeo.emission_factors(geos, flow=flow, b_consts=dict(b_r=1.0, b_th=0.0, b_ph=0.0), Q_frac=1.5, backend=backend)
        one = type(geos)({k: (np.asarray(v)[..., :1] if np.ndim(v) == 3 else v) for k, v in geos.items()})
        with pytest.raises(ValueError, match='too small to calculate a numerical gradient'):
            kgeo.emission_factors(one, flow=flow, backend=backend)
    with pytest.raises(ValueError, match='bogus'):
        kgeo.emission_factors(geos, flow=flow, backend='bogus')


def test_hip_backend_with_a_flow_needs_a_device_and_never_falls_back():
    import torch
    import __graft_entry__ as entry
    from bhnerf_amd import _hip
    entry.build()
    geos, ref = host_case('Zt')
    calls = (lambda: kgeo.emission_factors(geos, flow=ref['flow'], backend='hip'),
             lambda: kgeo.emission_factors(geos, flow=ref['umu'], b_consts=fc.b_consts_of('Zt'), backend='hip'),
             lambda: kgeo.emission_factors(geos, flow=ref['flow'], b_consts=fc.b_consts_of('Zt'), frame='zamo', backend='hip'))
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
    lib = _hip.flow_lib()
    p = 4096                                # never dereferenced: every call below is refused before a launch
    P = C.c_void_p(p)
    fields = gc.POINT_FIELDS + gc.RAY_FIELDS

    def record(**change):
        kw = dict(n=4, ngeo=8, spin=0.5, M=1.0, E=1.0, inc=1.0, omega=p, **{k: p for k in fields})
        kw.update(change)
        return _hip.bhn_flow_geos(kw['n'], kw['ngeo'], *[kw[k] for k in fields], kw['spin'], kw['M'], kw['E'], kw['inc'], kw['omega'])

    calls = {
        'zamo_velocity': lambda rec, a: lib.bhn_flow_zamo_velocity(rec, 0.5, 0.1, a.get('umu', P), None),
        'doppler': lambda rec, a: lib.bhn_flow_doppler(rec, a.get('umu', P), 0.0, 1, a.get('g', P), None),
        'fluid_field': lambda rec, a: lib.bhn_flow_fluid_field(rec, a.get('umu', P), 0.0, 1.0, 0.0, a.get('b', P), None),
        'transport': lambda rec, a: lib.bhn_flow_transport(rec, a.get('umu', P), a.get('g', P), a.get('b', P), a.get('divisor', None),
                                                            a.get('Q_frac', 0.5), 0.0, 1.0, a.get('J', P), None),
        'transport_zamo': lambda rec, a: lib.bhn_flow_transport_zamo(rec, 0.5, 0.1, a.get('g', P), a.get('b', P), a.get('divisor', None),
                                                                      a.get('Q_frac', 0.5), 1.0, a.get('J', P), None),
    }
    bad_records = [(None, b'null geos')] + [(record(**{k: None}), b'null field') for k in fields + ('omega',)] + [
        (record(n=0), b'ray count'), (record(n=-2), b'ray count'), (record(ngeo=1), b'ngeo must'), (record(ngeo=0), b'ngeo must'),
        (record(ngeo=-4), b'ngeo must'), (record(n=1 << 45, ngeo=1 << 20), b'too many points')]
    bad_args = {
        'zamo_velocity': [(dict(umu=None), b'null output umu')],
        'doppler': [(dict(umu=None), b'null umu'), (dict(g=None), b'null output')],
        'fluid_field': [(dict(umu=None), b'null umu'), (dict(b=None), b'null output')],
        'transport': [(dict(umu=None), b'null umu'), (dict(g=None), b'null g, b or J'), (dict(b=None), b'null g, b or J'),
                      (dict(J=None), b'null g, b or J'), (dict(Q_frac=1.5), b'Q_frac'), (dict(Q_frac=-0.1), b'Q_frac')],
        'transport_zamo': [(dict(g=None), b'null g, b or J'), (dict(b=None), b'null g, b or J'), (dict(J=None), b'null g, b or J'),
                           (dict(Q_frac=1.5), b'Q_frac'), (dict(Q_frac=-0.1), b'Q_frac')],
    }
    for name, call in calls.items():
        cases = [(C.byref(rec) if rec is not None else None, {}, word) for rec, word in bad_records]
        cases += [(C.byref(record()), change, word) for change, word in bad_args[name]]
        for rec, change, word in cases:
            rc = call(rec, change)
            assert rc == _hip.BHN_EINVAL, (name, change, word, rc)
            msg = lib.bhn_flow_last_error()
            assert msg and word in msg, (name, change, msg)
            with pytest.raises(_hip.HipError, match='libbhnerf_flow'):
                _hip.flow_check(rc)
    _hip.flow_check(0)


FLOW_NAMES = ['bhn_flow_doppler', 'bhn_flow_fluid_field', 'bhn_flow_last_error', 'bhn_flow_transport', 'bhn_flow_transport_zamo',
              'bhn_flow_zamo_velocity']


def test_flow_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_flow.so: the dynamic symbol table is the declarations of include/bhnerf_flow.h and nothing else, the ctypes table binds
    exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or ctypes table
    knows a name that begins with bhn_flow.  The sixth library has a tuple of its own: _hip.LIBRARIES keeps its five keys."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_flow.h'))))
    assert declared == sorted(_hip.FLOW_SIGNATURES) == FLOW_NAMES
    defined = side._symbols(_hip.FLOW_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.FLOW_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.FLOW_LIBRARY == (_hip.FLOW_LIB_PATH, _hip.FLOW_SIGNATURES, 'bhn_flow_last_error', None)
    assert _hip.flow_lib() is _hip.load(_hip.FLOW_LIB_PATH, _hip.FLOW_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    assert len(others) == 5
    for other_header, path, table in others:
        assert 'bhn_flow' not in side._header(other_header), other_header
        assert 'bhn_flow' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_flow') for k in table), other_header
    # and the new library knows no other library's names
    for prefix in ('bhn_kerr', 'bhn_eht', 'bhn_grf', 'bhn_eql'):
        assert prefix not in side._header('bhnerf_flow.h') and prefix not in defined, prefix
