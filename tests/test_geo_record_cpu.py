"""CPU tests of the geodesic-record library (libbhnerf_rec.so, csrc/geo_record.hip; geodesics.DeviceGeodesics and the resident mode):
everything about it that needs no device.

The per-point arithmetic lives in csrc/geo_record.h and compiles with a plain C++ compiler.  tools/geo_record_host.cpp is a stand-alone
program around it that runs the library's two passes (every point, then every ray's cumulative sum); here it is built with g++ -O2 and
the sanitizers (tests/side_lib_support.py), run as a child process on the host tracer's samples and compared with
geodesics._build_record on the same samples.  Nothing is loaded into this Python process but the library, for the argument checks.

Bounds.  r, theta, phi, t, mino, vr, vth and dtau are copies and sign flips of the samples: bitwise.  affine is bitwise
-np.cumsum(Sigma * dtau) of the program's OWN Sigma (the order of np.cumsum, no fused multiply-add).  The other fields differ from
NumPy's by the maths library's sin / cos / tan / pow: |got - want| <= GR_TOL max|want| per field (GR_TOL = 1e-10, the project's bound,
tests/gr_factor_cases.py), NaN and inf patterns equal; the measured figures are printed.  MEASURED (host build): Theta 2.8e-16, x / y / z at most
4.7e-19, Omega 1.1e-16, every other field (affine included) equal to _build_record's bit for bit.

Also here: the Keplerian Omega against the NumPy expression (r = 0, both senses of rotation), the ValueErrors of the resident mode,
DeviceGeodesics on CPU tensors, and the library's symbol table."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gr_factor_cases as gc                                           # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import alma, geodesics, kgeo                           # noqa: E402

BITWISE = ('r', 'theta', 'phi', 't', 'mino', 'vr', 'vth', 'dtau')
FIELDS = ('r', 'theta', 'phi', 't', 'mino', 'Delta', 'Sigma', 'Xi', 'omega', 'x', 'y', 'z', 'R', 'Theta', 'vr', 'vth', 'dtau', 'affine')
# name -> (spin, inclination, alpha, beta, ngeo): the 10 x 7 x 40 grid of gr_factor_cases' case A, one ray of one sample, one of three
SHAPES = {
    'grid': (0.94, np.deg2rad(60.0), None, None, gc.NGEO),
    'one': (0.94, np.deg2rad(60.0), [-6.0], [2.0], 1),
    'three': (0.5, np.deg2rad(30.0), [3.0], [-4.0], 3),
}
_SAMPLES = {}


def sampled(name):
    """(samples (7, n, ngeo), lam, eta, alpha, beta, spin, inc) of a shape on the host tracer, computed once and left unchanged."""
    if name not in _SAMPLES:
        spin, inc, alpha, beta, ngeo = SHAPES[name]
        if alpha is None:
            alpha, beta = np.meshgrid(np.linspace(*gc.FOV[0], gc.NA), np.linspace(*gc.FOV[1], gc.NB), indexing='ij')
        alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
        samp, lam, eta = geodesics._sample_rays(alpha.ravel(), beta.ravel(), spin, inc, 1000.0, 1.0, 0.02, 5.0, 400000, ngeo, 'numpy', None)
        _SAMPLES[name] = (samp, lam, eta, alpha, beta, spin, inc)
    return _SAMPLES[name]


def reference(name):
    samp, lam, eta, alpha, beta, spin, inc = sampled(name)
    out = {row: samp[i] for i, row in enumerate(geodesics.SAMPLE_ROWS)}
    with np.errstate(all='ignore'):
        return geodesics._build_record(out, lam, eta, alpha, beta, spin, inc, 1000.0, 1.0, 1.0)


def field_error(got, want, what):
    """max |got - want| / max |want| over the finite points, after the NaN / inf patterns are found equal."""
    gc.same_pattern(got, want, what)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    scale = np.abs(want[fin]).max()
    err = np.abs(got[fin] - want[fin]).max()
    return float(err / scale) if scale > 0.0 else (0.0 if err == 0.0 else np.inf)


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/geo_record_host.cpp built with the sanitizers -> a function (samples, lam, eta, spin, M, factor, rk) -> (fields, Omega)."""
    exe, work = side.build_host_program(tmp_path_factory, 'geo_record_host')

    def run(samples, lam, eta, spin, M, factor, rk, tag):
        _, n, ngeo = samples.shape
        rk = np.asarray(rk, dtype=np.float64).ravel()
        head = np.array([n, ngeo, spin, M, factor, rk.size], dtype=np.float64)
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        np.concatenate([head, samples.ravel(), lam.ravel(), eta.ravel(), rk]).tofile(fin)
        side.run_host(exe, fin, fout)
        raw = np.fromfile(fout, dtype=np.float64)
        assert raw.size == len(FIELDS) * n * ngeo + rk.size               # the documented sizes, nothing else
        fields = {k: raw[i * n * ngeo:(i + 1) * n * ngeo].reshape(n, ngeo) for i, k in enumerate(FIELDS)}
        return fields, raw[len(FIELDS) * n * ngeo:]
    return run


@pytest.mark.parametrize('name', list(SHAPES))
def test_host_build_of_the_point_code_equals_build_record(host_program, name):
    samp, lam, eta, alpha, beta, spin, inc = sampled(name)
    want = reference(name)
    got, _ = host_program(samp, lam, eta, spin, 1.0, 1.0, [], name)
    shape = want.r.shape
    assert samp.shape == (7, alpha.size, SHAPES[name][4]) and tuple(want.dims.values())[-1] == SHAPES[name][4]
    for k in BITWISE:
        assert got[k].reshape(shape).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    with np.errstate(all='ignore'):
        own = -np.cumsum(got['Sigma'] * got['dtau'], axis=-1)
    assert got['affine'].tobytes() == own.tobytes()                         # np.cumsum's order, no fused multiply-add
    errs = {k: field_error(got[k].reshape(shape), np.asarray(want[k]), k) for k in FIELDS if k not in BITWISE}
    print('\n[geo record, host build] %-5s %s  ' % (name, shape) + '  '.join('%s %.1e' % kv for kv in errs.items()))
    assert max(errs.values()) <= gc.GR_TOL, {k: e for k, e in errs.items() if e > gc.GR_TOL}


def test_host_build_of_the_keplerian_omega_equals_numpy(host_program):
    samp, lam, eta = sampled('three')[:3]
    rk = np.concatenate([[0.0, 1.0, 1e-300, 1e300, np.inf, np.nan], reference('grid').r.ravel()])
    for spin_k, M, factor in ((0.94, 1.0, 1.0), (0.94, 1.0, -0.7), (0.0, 1.0, -1.0), (-0.5, 2.5, 0.3)):
        _, Omega = host_program(samp, lam, eta, spin_k, M, factor, rk, 'kepler')
        sqrt_M = np.sqrt(M)
        with np.errstate(all='ignore'):
            want = factor * sqrt_M / (rk ** 1.5 + spin_k * sqrt_M)
        err = field_error(Omega, want, 'Omega')
        print('\n[geo record, host build] Omega spin %g M %g factor %g: %.1e, r = 0 gives %r' % (spin_k, M, factor, err, Omega[0]))
        assert err <= gc.GR_TOL
        assert Omega[0].tobytes() == want[0].tobytes()                     # r = 0: what NumPy gives (inf when spin = 0)
        assert np.array_equal(np.sign(Omega[np.isfinite(want)]), np.sign(want[np.isfinite(want)]))


# ---- argument checks, without a device

def test_argument_validation_returns_einval_before_any_device_call():
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.rec_lib()
    p = 4096                                # never dereferenced: every call below is refused before a launch
    P = C.c_void_p(p)

    def build(samples=P, lam=P, eta=P, n=4, ngeo=8, out=True, **null_field):
        fields = _hip.bhn_rec_fields(*[None if k in null_field else p for k in _hip.REC_FIELDS])
        return lib.bhn_rec_build(samples, lam, eta, n, ngeo, 0.5, 1.0, C.byref(fields) if out else None, None)

    cases = [(dict(samples=None), b'null samples'), (dict(lam=None), b'null lam or eta'), (dict(eta=None), b'null lam or eta'),
             (dict(out=False), b'null out'), (dict(n=0), b'ray count'), (dict(n=-3), b'ray count'), (dict(ngeo=0), b'ngeo must'),
             (dict(ngeo=-1), b'ngeo must'), (dict(n=1 << 45, ngeo=1 << 20), b'too many points')]
    cases += [({k: None}, b'null output field') for k in _hip.REC_FIELDS]
    for change, word in cases:
        rc = build(**change)
        assert rc == _hip.BHN_EINVAL, (change, rc)
        msg = lib.bhn_rec_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_rec'):
            _hip.rec_check(rc)
    kepler = [(lambda: lib.bhn_rec_kepler(None, 8, 0.5, 1.0, 1.0, P, None), b'null r'),
              (lambda: lib.bhn_rec_kepler(P, 8, 0.5, 1.0, 1.0, None, None), b'null output Omega'),
              (lambda: lib.bhn_rec_kepler(P, 0, 0.5, 1.0, 1.0, P, None), b'count must'),
              (lambda: lib.bhn_rec_kepler(P, -5, 0.5, 1.0, 1.0, P, None), b'count must'),
              (lambda: lib.bhn_rec_kepler(P, 1 << 60, 0.5, 1.0, 1.0, P, None), b'too many points')]
    for call, word in kepler:
        rc = call()
        assert rc == _hip.BHN_EINVAL, (word, rc)
        assert word in lib.bhn_rec_last_error(), (word, lib.bhn_rec_last_error())
    _hip.rec_check(0)


# ---- host logic

def test_resident_needs_the_hip_backend_before_anything_touches_a_device():
    with pytest.raises(ValueError, match="resident=True .* needs backend='hip'"):
        geodesics.image_plane_geos(0.5, 1.0, (-5.0, 5.0), (-5.0, 5.0), ngeo=4, num_alpha=2, num_beta=2, resident=True)
    with pytest.raises(ValueError, match="resident=True .* needs backend='hip'"):
        geodesics.ray_geos(0.5, 1.0, [1.0], [2.0], ngeo=4, backend='numpy', resident=True)
    with pytest.raises(ValueError, match='bogus'):                         # the backend's own error comes first
        geodesics.ray_geos(0.5, 1.0, [1.0], [2.0], ngeo=4, backend='bogus', resident=True)


@pytest.mark.parametrize('backends', [{}, dict(tracer='hip'), dict(factors='hip'), dict(tracer='numpy', factors='hip')])
def test_params_resident_needs_both_hip_back_ends(backends):
    params = dict(num_alpha=2, num_beta=2, fov_M=10.0, z_width=4.0, rmin='ISCO', Q_frac=0.5, b_consts=dict(arad=0.0, avert=1.0, ator=0.0),
                  Omega_dir='cw', t_start_obs=9.0, resident=True, **backends)
    with pytest.raises(ValueError, match="params\\['resident'\\] needs"):
        alma.image_plane_model(1.0, 0.5, params)
    with pytest.raises(ValueError, match="params\\['resident'\\] needs"):
        alma.get_raytracing_args(1.0, 0.5, params)


def test_device_geodesics_on_cpu_tensors():
    want = reference('three')
    want['r'] = want['r'].copy()
    want['r'][0, 1] = np.nan
    want['R'] = want['R'].copy()
    want['R'][0, 0], want['R'][0, 2] = np.inf, -np.inf
    rec = geodesics.DeviceGeodesics((k, torch.as_tensor(v) if isinstance(v, np.ndarray) else v) for k, v in want.items())
    assert isinstance(rec, geodesics.Geodesics) and rec.device == torch.device('cpu') and rec.dims == want.dims
    assert list(rec) == list(want)
    filled = rec.fillna(0.0)
    assert isinstance(filled, geodesics.DeviceGeodesics) and list(filled) == list(want)
    assert torch.isnan(rec.r[0, 1]) and filled.r is not rec.r              # a copy: the record itself is unchanged
    back, ref = filled.numpy(), want.fillna(0.0)
    assert type(back) is geodesics.Geodesics and list(back) == list(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert isinstance(filled[k], torch.Tensor) and filled[k].dtype == torch.float64
            assert back[k].dtype == np.float64 and back[k].shape == v.shape and back[k].tobytes() == v.tobytes(), k      # NaN only: the infs stay
        else:
            assert isinstance(filled[k], float) and back[k] == v, k
    assert back.r[0, 1] == 0.0 and back.R[0, 0] == np.inf and back.R[0, 2] == -np.inf
    with pytest.raises(ValueError, match=r'\.numpy\(\)'):
        kgeo.emission_factors(rec, 0.1, backend='numpy')


def test_rotate_evpa_on_a_tensor_gives_numpys_bits():
    from bhnerf_amd import emission
    rng = np.random.default_rng(5)
    J = rng.normal(size=(3, 4, 5, 6))
    J[1, 0, 0, 0], J[2, 1, 1, 1] = np.inf, np.nan
    for angle in (0.0, 0.3, -1.2):
        with np.errstate(all='ignore'):
            want = emission.rotate_evpa(J, angle)
        got = emission.rotate_evpa(torch.as_tensor(J), angle)
        assert isinstance(got, torch.Tensor) and got.numpy().tobytes() == want.tobytes(), angle
    qu = rng.normal(size=(7, 2))
    assert emission.rotate_evpa(torch.as_tensor(qu), 0.4, axis=1).numpy().tobytes() == emission.rotate_evpa(qu, 0.4, axis=1).tobytes()


# ---- conventions

REC_NAMES = ['bhn_rec_build', 'bhn_rec_kepler', 'bhn_rec_last_error']


def test_rec_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_rec.so: the dynamic symbol table is the declarations of include/bhnerf_rec.h and nothing else, the ctypes table binds
    exactly those, the library references no allocator, no getenv and no synchronisation, and none of the other six libraries, headers
    or ctypes tables knows a name that begins with bhn_rec_.  The seventh library has a tuple of its own: _hip.LIBRARIES keeps its
    five keys."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_rec.h'))))
    assert declared == sorted(_hip.REC_SIGNATURES) == REC_NAMES
    defined = side._symbols(_hip.REC_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.REC_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.REC_LIBRARY == (_hip.REC_LIB_PATH, _hip.REC_SIGNATURES, 'bhn_rec_last_error', None)
    assert _hip.rec_lib() is _hip.load(_hip.REC_LIB_PATH, _hip.REC_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    others.append(('bhnerf_flow.h', _hip.FLOW_LIB_PATH, _hip.FLOW_SIGNATURES))
    assert len(others) == 6
    for other_header, path, table in others:
        assert 'bhn_rec_' not in side._header(other_header), other_header
        assert 'bhn_rec_' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_rec_') for k in table), other_header
    # and the new library knows no other library's names
    for prefix in ('bhn_kerr', 'bhn_eht', 'bhn_grf', 'bhn_eql', 'bhn_flow'):
        assert prefix not in side._header('bhnerf_rec.h') and prefix not in defined, prefix
    # the struct of the 18 outputs is the header's, field for field
    text = side._header('bhnerf_rec.h')
    names = re.search(r'typedef struct bhn_rec_fields \{\s*double ([^;]*);', text).group(1)
    assert tuple(n.strip().lstrip('*') for n in names.split(',')) == _hip.REC_FIELDS == tuple(k for k, _ in _hip.bhn_rec_fields._fields_)
    assert _hip.REC_FIELDS == FIELDS
