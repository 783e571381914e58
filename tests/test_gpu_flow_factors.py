"""GPU tests of the general-flow (g, J) library on the device (libbhnerf_flow.so, csrc/flow_factors.hip; kgeo.emission_factors with
flow= and backend='hip').

Device against the NumPy functions of kgeo.py composed directly, on the cases, by the metric and at the bound of
tests/flow_factor_cases.py and tests/gr_factor_cases.py (GR_TOL = 1e-10; NaN and inf patterns identical at every point), in both
tetrads.  The records come from the device tracer (image_plane_geos(backend='hip')); the reference is computed from the same record,
once per case.  The kernels restate kgeo.py expression for expression, so the two differ by the device's sin / cos / atan2 / pow /
sqrt only; the per-case maxima are printed.  MEASURED on the MI355X: see DESIGN.md 4.13.

Also: two launches give the same bytes, a subset of the rays gives the bytes of its columns, the scalar ZAMO path against the same
velocity handed over as an array, the caller-owned-buffer contract (guard bands, poisoned outputs, read-only inputs, in the style of
tests/test_gpu_gr_factors.py), and the polarised-ring study's flow end to end at small size."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_factor_cases as fc                                         # noqa: E402
import gr_factor_cases as gc                                           # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401
from bhnerf_amd import _hip, emission, kgeo                            # noqa: E402

pytestmark = pytest.mark.gpu

POINT_FIELDS = gc.POINT_FIELDS + ('omega',)
_CASES = {}


def case(name, dev, V_frac=0.0, spectral_index=1):
    """(record, reference) of a case on the device tracer's record, computed once and left unchanged.  The V variant divides the field
    by its domain mean (NumPy's), the others take it as it is."""
    record = fc.CASES[name][0]
    if record not in _CASES:
        _CASES[record] = gc.trace(record, backend='hip', device=dev)
    key = (name, V_frac, spectral_index)
    if key not in _CASES:
        divisor = fc.domain_mean(case(name, dev)[1]) if V_frac != 0 else None
        _CASES[key] = fc.reference(name, _CASES[record], V_frac, spectral_index, divisor)
    return _CASES[record], _CASES[key]


class DeviceRecord:
    """The fields of a record (rays `rays` of it, all by default) on the device and the struct that names them."""

    def __init__(self, geos, dev, rays=slice(None)):
        self.ngeo = geos.r.shape[-1]
        self.rays, self.dev = rays, dev
        self.t = {k: self.place(geos[k], self.ngeo) for k in POINT_FIELDS}
        self.t.update({k: self.place(geos[k], 1) for k in gc.RAY_FIELDS})
        self.n = self.t['r'].shape[0]
        self.rec = _hip.bhn_flow_geos(self.n, self.ngeo, *[self.t[k].data_ptr() for k in gc.POINT_FIELDS + gc.RAY_FIELDS],
                                      float(geos.spin), float(geos.M), float(geos.E), float(geos.inc), self.t['omega'].data_ptr())
        self.ref = C.byref(self.rec)
        self.total = self.n * self.ngeo

    def place(self, v, width):
        """(rays, width) of a per-point or per-ray array (width 4 ngeo: a umu array, 3 ngeo: a field) on the device."""
        return torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, width)[self.rays]), device=self.dev)


def run_library(d, flow, field, dev, fill=True, V_frac=0.0, spectral_index=1, zamo_frame=False, divisor=None, out=None):
    """The calls on a DeviceRecord: a dict of NumPy arrays umu (a scalar flow only), g, b (a field dict only), J.  flow: ('zamo', beta,
    chi) or a umu array; field: dict(arad, avert, ator) or a b array.  `out`: data pointers for the outputs (the guard-band test's),
    torch allocations otherwise."""
    lib, stream = _hip.flow_lib(), _hip.stream_ptr(dev)
    S = 4 if (V_frac != 0 and not zamo_frame) else 3
    scalar, fluid = isinstance(flow, tuple), isinstance(field, dict)
    sizes = output_sizes(d, scalar, fluid, S)
    keep = None
    if out is None:
        keep = {k: torch.empty(size, dtype=torch.float64, device=dev) for k, size in sizes.items()}
        out = {k: _hip.ptr(v) for k, v in keep.items()}
    inputs = {}
    if not scalar:
        inputs['umu'] = d.place(flow, 4 * d.ngeo)
    if not fluid:
        inputs['b'] = d.place(field, 3 * d.ngeo)
    before = {k: v.clone() for k, v in inputs.items()}
    umu = out['umu'] if scalar else _hip.ptr(inputs['umu'])
    b = out['b'] if fluid else _hip.ptr(inputs['b'])
    if scalar:
        _hip.flow_check(lib.bhn_flow_zamo_velocity(d.ref, flow[1], flow[2], umu, stream))
    _hip.flow_check(lib.bhn_flow_doppler(d.ref, umu, 0.0, 1 if fill else 0, out['g'], stream))
    if fluid:
        _hip.flow_check(lib.bhn_flow_fluid_field(d.ref, umu, field['arad'], field['avert'], field['ator'], b, stream))
    div_t = None if divisor is None else torch.full((1,), divisor, dtype=torch.float64, device=dev)
    if zamo_frame:
        _hip.flow_check(lib.bhn_flow_transport_zamo(d.ref, flow[1], flow[2], out['g'], b, _hip.ptr(div_t), fc.Q_FRAC, float(spectral_index),
                                                    out['J'], stream))
    else:
        _hip.flow_check(lib.bhn_flow_transport(d.ref, umu, out['g'], b, _hip.ptr(div_t), fc.Q_FRAC, V_frac, float(spectral_index), out['J'],
                                               stream))
    torch.cuda.synchronize(dev)
    assert all(torch.equal(inputs[k].view(torch.int64), before[k].view(torch.int64)) for k in inputs)      # read-only inputs (NaN included)
    if keep is None:
        return None
    shape = (d.n, d.ngeo)
    shapes = dict(umu=shape + (4,), g=shape, b=shape + (3,), J=(S,) + shape)
    return {k: (keep[k].cpu().numpy().reshape(shapes[k]) if k in keep else None) for k in shapes}


def output_sizes(d, scalar, fluid, S):
    """name -> float64 elements of the outputs the library writes for this kind of flow and field."""
    sizes = dict(g=d.total, J=S * d.total)
    if scalar:
        sizes['umu'] = 4 * d.total
    if fluid:
        sizes['b'] = 3 * d.total
    return sizes


def field_for_library(name, ref):
    return fc.b_consts_of(name) if fc.CASES[name][3] == 'fluid' else ref['b']


def shaped(out, shape):
    return {k: (None if v is None else v.reshape({'umu': shape + (4,), 'g': shape, 'b': shape + (3,)}.get(k, (v.shape[0],) + shape)))
            for k, v in out.items()}


@pytest.mark.parametrize('name,V_frac,spectral_index', fc.VARIANTS)
def test_device_equals_the_numpy_functions(dev, name, V_frac, spectral_index):
    geos, ref = case(name, dev, V_frac, spectral_index)
    fc.assert_conditions(name, geos, ref)
    shape = geos.r.shape
    d = DeviceRecord(geos, dev)
    flow, field, kw = ref['flow'], field_for_library(name, ref), dict(V_frac=V_frac, spectral_index=spectral_index, divisor=ref['divisor'])
    out = shaped(run_library(d, flow, field, dev, True, **kw), shape)
    g_nan = run_library(d, flow, field, dev, False, **kw)['g'].reshape(shape)
    zamo = shaped(run_library(d, flow, field, dev, True, zamo_frame=True, **kw), shape) if name in fc.SCALAR else None
    errs = fc.errors(ref, umu=out['umu'], g=out['g'], g_nan=g_nan, b=out['b'], J=out['J'], J_zamo=zamo and zamo['J'])
    fc.report('device vs host', name, V_frac, spectral_index, errs)
    assert max(errs.values()) <= fc.GR_TOL, (name, {k: e for k, e in errs.items() if e > fc.GR_TOL})
    # the Python surface: the bytes the library wrote (no domain), or, with the domain of the V variant, the device's own mean
    py = dict(Q_frac=fc.Q_FRAC, V_frac=V_frac, spectral_index=spectral_index, backend='hip', device=dev)
    domain = None if ref['divisor'] is None else fc.domain_of(name)
    g_py, J_py = kgeo.emission_factors(geos, flow=flow, b_consts=fc.b_consts_of(name), domain=domain, **py)
    assert g_py.shape == shape and J_py.shape == out['J'].shape and g_py.dtype == J_py.dtype == np.float64
    assert g_py.tobytes() == out['g'].tobytes()
    g_only, none = kgeo.emission_factors(geos, flow=flow, fillna=False, backend='hip', device=dev)
    assert none is None and g_only.tobytes() == g_nan.tobytes()
    Jz_py = kgeo.emission_factors(geos, flow=flow, b_consts=fc.b_consts_of(name), domain=domain, frame='zamo', **py)[1] if zamo else None
    if domain is None:
        assert J_py.tobytes() == out['J'].tobytes() and (zamo is None or Jz_py.tobytes() == zamo['J'].tobytes())
    else:
        errs = fc.errors(ref, J=J_py, J_zamo=Jz_py)
        fc.report('device with its own domain mean', name, V_frac, spectral_index, errs)
        assert max(errs.values()) <= fc.GR_TOL, errs
    if name in fc.SCALAR:                                               # an array field reaches the device as it is
        g_arr, J_arr = kgeo.emission_factors(geos, flow=flow, b_consts=ref['b'], domain=domain, **py)
        errs = fc.errors(ref, g=g_arr, J=J_arr)
        assert max(errs.values()) <= fc.GR_TOL, errs


def test_two_launches_and_a_subset_of_the_rays_give_the_same_bytes(dev):
    geos, ref = case('Z3', dev)
    flow, field = ref['flow'], fc.b_consts_of('Z3')
    full = DeviceRecord(geos, dev)
    for zamo_frame in (False, True):
        one = run_library(full, flow, field, dev, zamo_frame=zamo_frame)
        two = run_library(full, flow, field, dev, zamo_frame=zamo_frame)
        assert all(one[k].tobytes() == two[k].tobytes() for k in one)
        sub = slice(5, 13)                                              # rays 5..12 alone: other lanes, another n, the same bytes
        part = DeviceRecord(geos, dev, rays=sub)
        assert (part.n, part.ngeo) == (8, gc.NGEO)
        div = run_library(full, flow, field, dev, zamo_frame=zamo_frame, divisor=1.7)
        got = run_library(part, flow, field, dev, zamo_frame=zamo_frame, divisor=1.7)
        for k in ('umu', 'g', 'b'):
            assert got[k].tobytes() == np.ascontiguousarray(div[k][sub]).tobytes(), k
        assert got['J'].tobytes() == np.ascontiguousarray(div['J'][:, sub]).tobytes()
        assert not np.array_equal(div['J'], one['J'], equal_nan=True)   # the divisor is read


def test_the_scalar_zamo_path_and_the_same_velocity_as_an_array_agree(dev):
    geos, ref = case('Z1', dev, 0.01, 1.5)
    shape = geos.r.shape
    d = DeviceRecord(geos, dev)
    kw = dict(V_frac=0.01, spectral_index=1.5, divisor=ref['divisor'])
    scalar = shaped(run_library(d, ref['flow'], ref['b'], dev, **kw), shape)
    array = shaped(run_library(d, ref['umu'], ref['b'], dev, **kw), shape)          # NumPy's zamo_frame_velocity, handed over
    assert array['umu'] is None
    want = dict(ref, g=scalar['g'], J=scalar['J'])
    errs = fc.errors(want, g=array['g'], J=array['J'])
    bitwise = {k: array[k].tobytes() == scalar[k].tobytes() for k in ('g', 'J')}
    print('\n[flow factors, device] scalar ZAMO path against the umu array of the host: %s; bitwise %s; device umu == host umu: %s'
          % ('  '.join('%s %.1e' % kv for kv in errs.items()), bitwise, np.array_equal(scalar['umu'], ref['umu'])))
    assert max(errs.values()) <= fc.GR_TOL, errs


# ---- caller-owned buffers

GUARD = 1 << 16
FILLS = (0xFF, 0x7F)            # NaN as float64;  1.4e306 as float64


@pytest.mark.parametrize('name,V_frac,zamo_frame', [('Z1', 0.01, False), ('Z1', 0.01, True), ('Z3', 0.0, False), ('Zs', 0.0, False),
                                                    ('Zt', 0.0, False), ('Zt', 0.0, True)])
def test_guard_bands_stay_intact_and_every_output_element_is_written(dev, name, V_frac, zamo_frame):
    """Z1 with the V row, Z3 (the field kernel), Zs (the library itself writes NaN there) and the one-ray case (a tail workgroup only)."""
    geos, ref = case(name, dev, V_frac, 1.5 if V_frac else 1)
    flow, field = ref['flow'], field_for_library(name, ref)
    d = DeviceRecord(geos, dev)
    before = {k: v.clone() for k, v in d.t.items()}
    S = 4 if (V_frac != 0 and not zamo_frame) else 3
    kw = dict(V_frac=V_frac, spectral_index=1.5 if V_frac else 1, zamo_frame=zamo_frame, divisor=ref['divisor'])
    results = {}
    for fill in FILLS:
        sizes = output_sizes(d, isinstance(flow, tuple), isinstance(field, dict), S)
        bufs = {k: Guarded(k, 8 * size, fill, dev, guard=GUARD) for k, size in sizes.items()}
        run_library(d, flow, field, dev, True, out={k: v.ptr for k, v in bufs.items()}, **kw)
        bad = [m for m in (v.disturbed() for v in bufs.values()) if m]
        assert not bad, 'fill 0x%02X: %s' % (fill, '; '.join(bad))
        assert all(torch.equal(d.t[k], before[k]) for k in before)                    # read-only inputs
        for k, v in bufs.items():                                                     # (a NaN of the library's is never eight 0xFF bytes)
            assert v.poisoned(8) == 0, 'fill 0x%02X: %d elements of %s were not written' % (fill, v.poisoned(8), k)
        results[fill] = {k: v.mid.cpu().numpy().tobytes() for k, v in bufs.items()}
    assert results[FILLS[0]] == results[FILLS[1]]                       # nothing depends on what the buffers held
    out = run_library(d, flow, field, dev, True, **kw)
    assert all(out[k].tobytes() == results[0x7F][k] for k in results[0x7F])


# ---- the polarised-ring study's flow

def test_the_ring_study_end_to_end_at_small_size(dev):
    spin, inc, distance = 0.94, np.deg2rad(60.0), 200.0
    varphis = np.deg2rad(np.linspace(5.0, 320.0, 8))
    _, _, alpha, beta = kgeo.equatorial_lensing.rho_of_req(spin, inc, 5.0, mbar=0, varphis=varphis, distance=distance, backend='hip', device=dev)
    geos = kgeo.ray_geos(spin, inc, alpha, beta, ngeo=40, distance=distance, backend='hip', device=dev).fillna(0.0)
    assert geos.r.shape == (8, 40)
    kw = dict(flow=('zamo', 0.5, -np.pi / 2), b_consts=dict(b_r=0.87, b_th=0.0, b_ph=0.5), V_frac=0)
    g, J = kgeo.emission_factors(geos, backend='hip', device=dev, **kw)
    with np.errstate(all='ignore'):
        g_np, J_np = kgeo.emission_factors(geos, backend='numpy', **kw)
    z_width, rmin, rmax = gc.domain_of('A')                             # the same hole: spin 0.94
    domain = (np.abs(geos.z) < z_width) & (geos.r > rmin) & (geos.r < rmax)
    assert domain.sum() >= 24
    gc.same_pattern(g, g_np, 'g')
    errs = {'g': float(np.abs(g - g_np).max() / np.abs(g_np).max())}
    errs.update({'J%d' % s: gc.plane_error(J[s], J_np[s], domain, 'J[%d]' % s) for s in range(3)})
    print('\n[flow factors, ring study] ' + '  '.join('%s %.1e' % kv for kv in errs.items()))
    assert J.shape == (3, 8, 40) and max(errs.values()) <= fc.GR_TOL, errs
    ring = emission.equatorial_ring(geos, 0, backend='hip', device=dev)
    assert ring.sum() == 8.0                                            # every ray of rho_of_req meets the plane
    stokes = (g ** 2 * ring * np.nan_to_num(J) * np.asarray(geos.Sigma)).sum(axis=-1)
    print('    Stokes sums of the 8 rays: I %s\n    Q %s\n    U %s' % tuple(stokes))
    assert stokes.shape == (3, 8) and np.isfinite(stokes).all() and (stokes[0] > 0).all() and (stokes[1:] != 0).any(axis=1).all()
