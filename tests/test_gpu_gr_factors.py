"""GPU tests of the (g, J) library on the device (libbhnerf_grf.so, csrc/gr_factors.hip; kgeo.emission_factors with backend='hip').

Device against the NumPy functions of kgeo.py, composed as alma.image_plane_model composes them, on the cases, by the metric and at the
bound of tests/gr_factor_cases.py (GR_TOL = 1e-10; NaN and inf patterns identical at every point).  The records come from the
device tracer (image_plane_geos(backend='hip')); the reference is computed from the same record, once per case.  The kernels
restate kgeo.py expression for expression, so the two differ by the device's sin / cos / atan2 / pow only; the per-case maxima are
printed.  MEASURED on the MI355X: see DESIGN.md 4.11.

Also: two launches give the same bytes, a subset of the rays gives the bytes of its columns, the caller-owned-buffer contract
(guard bands, poisoned outputs and workspace, in the style of tests/test_gpu_kerr_trace.py), and the way through
alma.get_raytracing_args into a training step."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gr_factor_cases as gc                                           # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401
from bhnerf_amd import _hip, kgeo                                      # noqa: E402

pytestmark = pytest.mark.gpu


_CASES = {}


def case(name, dev, V_frac=0.0, spectral_index=1):
    """(record, reference) of a case on the device tracer's record, computed once and left unchanged."""
    if name not in _CASES:
        _CASES[name] = gc.trace(name, backend='hip', device=dev)
    key = (name, V_frac, spectral_index)
    if key not in _CASES:
        _CASES[key] = gc.reference(name, _CASES[name], V_frac, spectral_index)
    return _CASES[name], _CASES[key]


class DeviceRecord:
    """The fields of a record (rays `rays` of it, all by default) on the device and the struct that names them."""

    def __init__(self, geos, Omega, dev, rays=slice(None)):
        ngeo = geos.r.shape[-1]
        flat = lambda v, width: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, width)[rays])
        self.t = {k: torch.as_tensor(flat(geos[k], ngeo), device=dev) for k in gc.POINT_FIELDS}
        self.t.update({k: torch.as_tensor(flat(geos[k], 1), device=dev) for k in gc.RAY_FIELDS})
        self.Omega = torch.as_tensor(flat(Omega, ngeo), device=dev)
        self.n, self.ngeo = self.Omega.shape
        self.rec = _hip.bhn_grf_geos(self.n, self.ngeo, *[self.t[k].data_ptr() for k in gc.POINT_FIELDS + gc.RAY_FIELDS],
                                     float(geos.spin), float(geos.M), float(geos.E), float(geos.inc))
        self.ref = C.byref(self.rec)
        self.total = self.n * self.ngeo


def run_library(d, field, domain, dev, fill=True, V_frac=0.0, spectral_index=1, divisor=None, out=None):
    """The four calls on a DeviceRecord: NumPy (g, b, mean, J).  `divisor`: a float to divide b by instead of the domain mean.
    `out`: data pointers for g, b, mean, ws, J (the guard-band test's), torch allocations otherwise."""
    lib, stream = _hip.grf_lib(), _hip.stream_ptr(dev)
    S = 4 if V_frac != 0 else 3
    ws_bytes = int(lib.bhn_grf_ws_bytes(d.n, d.ngeo))
    assert ws_bytes == 16 * ((d.total + 255) // 256)
    keep = None
    if out is None:
        keep = dict(g=torch.empty(d.total, dtype=torch.float64, device=dev), b=torch.empty(3 * d.total, dtype=torch.float64, device=dev),
                    mean=torch.empty(1, dtype=torch.float64, device=dev), ws=torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev),
                    J=torch.empty(S * d.total, dtype=torch.float64, device=dev))
        out = {k: _hip.ptr(v) for k, v in keep.items()}
    _hip.grf_check(lib.bhn_grf_doppler(d.ref, _hip.ptr(d.Omega), 0.0, 1 if fill else 0, out['g'], stream))
    _hip.grf_check(lib.bhn_grf_fluid_field(d.ref, _hip.ptr(d.Omega), field[0], field[1], field[2], out['b'], stream))
    _hip.grf_check(lib.bhn_grf_domain_mean(d.ref, out['b'], domain[0], domain[1], domain[2], out['mean'], out['ws'], ws_bytes, stream))
    div_t = None if divisor is None else torch.full((1,), divisor, dtype=torch.float64, device=dev)
    div = out['mean'] if divisor is None else _hip.ptr(div_t)
    _hip.grf_check(lib.bhn_grf_transport(d.ref, _hip.ptr(d.Omega), out['g'], out['b'], div, gc.Q_FRAC, V_frac, float(spectral_index), out['J'],
                                         stream))
    torch.cuda.synchronize(dev)
    if keep is None:
        return None
    shape = (d.n, d.ngeo)
    return (keep['g'].cpu().numpy().reshape(shape), keep['b'].cpu().numpy().reshape(shape + (3,)), float(keep['mean'].cpu()[0]),
            keep['J'].cpu().numpy().reshape((S,) + shape))


@pytest.mark.parametrize('name,V_frac,spectral_index', gc.VARIANTS)
def test_device_equals_the_numpy_functions(dev, name, V_frac, spectral_index):
    geos, ref = case(name, dev, V_frac, spectral_index)
    gc.assert_conditions(name, ref)
    shape = geos.r.shape
    d = DeviceRecord(geos, ref['Omega'], dev)
    g, b, mean, J = run_library(d, gc.CASES[name][3], gc.domain_of(name), dev, True, V_frac, spectral_index)
    g_nan = run_library(d, gc.CASES[name][3], gc.domain_of(name), dev, False, V_frac, spectral_index)[0]
    errs = gc.errors(g.reshape(shape), b.reshape(shape + (3,)), mean, J.reshape((-1,) + shape), ref, got_g_nan=g_nan.reshape(shape))
    gc.report('device vs host', name, V_frac, spectral_index, errs)
    assert max(errs.values()) <= gc.GR_TOL, (name, {k: e for k, e in errs.items() if e > gc.GR_TOL})
    # the Python surface returns what the library wrote
    consts = dict(zip(('arad', 'avert', 'ator'), gc.CASES[name][3]))
    g_py, J_py = kgeo.emission_factors(geos, ref['Omega'], consts, gc.domain_of(name), Q_frac=gc.Q_FRAC, V_frac=V_frac,
                                       spectral_index=spectral_index, backend='hip', device=dev)
    assert g_py.shape == shape and J_py.shape == J.shape[:1] + shape and g_py.dtype == J_py.dtype == np.float64
    assert g_py.tobytes() == g.tobytes() and J_py.tobytes() == J.tobytes()
    g_only, none = kgeo.emission_factors(geos, ref['Omega'], fillna=False, backend='hip', device=dev)
    assert none is None and g_only.tobytes() == g_nan.tobytes()


def test_two_launches_and_a_subset_of_the_rays_give_the_same_bytes(dev):
    geos, ref = case('A', dev)
    field, domain = gc.CASES['A'][3], gc.domain_of('A')
    full = DeviceRecord(geos, ref['Omega'], dev)
    g, b, mean, J = run_library(full, field, domain, dev)
    g2, b2, mean2, J2 = run_library(full, field, domain, dev)
    assert g.tobytes() == g2.tobytes() and b.tobytes() == b2.tobytes() and J.tobytes() == J2.tobytes()
    assert np.float64(mean).tobytes() == np.float64(mean2).tobytes()
    sub = slice(5, 13)                                                  # rays 5..12 alone: other lanes, another n, the same bytes
    part = DeviceRecord(geos, ref['Omega'], dev, rays=sub)
    assert (part.n, part.ngeo) == (8, gc.NGEO)
    _, _, _, J_div = run_library(full, field, domain, dev, divisor=1.7)
    g_s, b_s, _, J_s = run_library(part, field, domain, dev, divisor=1.7)
    assert g_s.tobytes() == np.ascontiguousarray(g[sub]).tobytes()
    assert b_s.tobytes() == np.ascontiguousarray(b[sub]).tobytes()
    assert J_s.tobytes() == np.ascontiguousarray(J_div[:, sub]).tobytes()
    assert not np.array_equal(J_div, J, equal_nan=True)                 # the divisor is read


# ---- caller-owned buffers

GUARD = 1 << 16
FILLS = (0xFF, 0x7F)            # NaN as float64;  1.4e306 as float64


@pytest.mark.parametrize('name,V_frac', [('B', 0.01), ('C', 0.0), ('tiny', 0.0)])
def test_guard_bands_stay_intact_and_every_output_element_is_written(dev, name, V_frac):
    """Case B with the V row, case C (the library itself writes NaN there) and the one-ray case (a tail workgroup only)."""
    geos, ref = case(name, dev, V_frac, 1)
    field, domain = gc.CASES[name][3], gc.domain_of(name)
    d = DeviceRecord(geos, ref['Omega'], dev)
    before = {k: v.clone() for k, v in d.t.items()}
    S = 4 if V_frac != 0 else 3
    blocks = (d.total + 255) // 256
    results = {}
    for fill in FILLS:
        sizes = dict(g=8 * d.total, b=8 * 3 * d.total, mean=8, ws=16 * blocks, J=8 * S * d.total)
        bufs = {k: Guarded(k, nbytes, fill, dev, guard=GUARD) for k, nbytes in sizes.items()}
        run_library(d, field, domain, dev, True, V_frac, 1, out={k: v.ptr for k, v in bufs.items()})
        bad = [m for m in (v.disturbed() for v in bufs.values()) if m]
        assert not bad, 'fill 0x%02X: %s' % (fill, '; '.join(bad))
        assert all(torch.equal(d.t[k], before[k]) for k in before)                    # read-only inputs
        for k, v in bufs.items():                                                     # (a NaN of the library's is never eight 0xFF bytes)
            assert v.poisoned(8) == 0, 'fill 0x%02X: %d elements of %s were not written' % (fill, v.poisoned(8), k)
        results[fill] = {k: v.mid.cpu().numpy().tobytes() for k, v in bufs.items()}
    assert results[FILLS[0]] == results[FILLS[1]]                       # nothing depends on what the buffers held, the workspace included
    g, b, mean, J = run_library(d, field, domain, dev, True, V_frac, 1)
    assert g.tobytes() == results[0x7F]['g'] and b.tobytes() == results[0x7F]['b'] and J.tobytes() == results[0x7F]['J']
    assert np.float64(mean).tobytes() == results[0x7F]['mean']


# ---- through the ALMA glue

def test_alma_raytracing_args_with_the_hip_factors_feed_a_training_step(dev):
    from bhnerf_amd import alma, network, optimization, units
    params = dict(fov_M=40.0, z_width=4, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0, avert=1, ator=0), Omega_dir='cw',
                  num_alpha=8, num_beta=8, t_start_obs=9.3, tracer='hip')
    rt_np = alma.get_raytracing_args(np.deg2rad(12.0), 0.0, dict(params, factors='numpy'))
    rt = alma.get_raytracing_args(np.deg2rad(12.0), 0.0, dict(params, factors='hip'))
    assert len(rt) == len(rt_np) == 1 and list(rt[0]) == list(rt_np[0])
    for k in rt[0]:
        assert type(rt[0][k]) is type(rt_np[0][k]), k
        g, w = np.asarray(units.strip(rt[0][k])), np.asarray(units.strip(rt_np[0][k]))
        assert g.shape == w.shape and g.dtype == w.dtype, k
        assert np.isfinite(g).all() and np.allclose(g, w, rtol=1e-6, atol=1e-6 * (np.abs(w).max() or 1.0)), k
    assert np.abs(rt[0]['J']).max() > 0.0
    t = (9.3 + np.linspace(0.05, 0.5, 4)) * units.hr
    data = np.abs(np.random.default_rng(3).standard_normal((4, 3))) * 1e-2
    pred = network.NeRF_Predictor(20.0, 6.0, 20.0, 4.0, net_depth=4, net_width=64, mode='f32', device=dev)
    step = optimization.TrainStep.image(t, data, sigma=1e-2, dtype='lc')
    opt = optimization.Optimizer({'num_iters': 1, 'lr_init': 1e-3, 'lr_final': 1e-4}, pred, rt)
    opt.run(4, step, rt)
    assert opt.state.step == 1 and np.isfinite(float(np.mean(opt.loss)))
