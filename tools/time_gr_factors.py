#!/usr/bin/env python3
"""Time kgeo.emission_factors (Doppler factor g and polarised transport factors J of one hypothesis) on both back ends, in one
process, and write profiles/gr_factors_time.txt.

    python tools/time_gr_factors.py [--out profiles/gr_factors_time.txt]

Per ray set (64 x 64 rays x 100 samples and 128 x 128 x 64, traced on the GPU, spin 0.94, 60 deg, ccw Keplerian, vertical field,
the domain of alma.image_plane_model): 'numpy' is the wall time of the composed host functions (median of 3); 'hip' the wall time
of the same call with backend='hip' after a warm-up (median of 5; upload of the fields and download of g and J included), and the
four library calls alone between two HIP events on fields already on the device (median of 5).  No threshold: figures only."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bhnerf_amd import _hip, constants, kgeo                         # noqa: E402

SPIN, INC, FOV = 0.94, np.deg2rad(60.0), 40.0
CONSTS = dict(arad=0.0, avert=1.0, ator=0.0)
POINT_FIELDS = ('r', 'theta', 'affine', 'Delta', 'Sigma', 'Xi', 'R', 'Theta')
RAY_FIELDS = ('lam', 'alpha', 'beta')


def wall(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def library_calls_ms(geos, Omega, domain, dev, repeats=5):
    """The four library calls alone (doppler, fluid_field, domain_mean, transport) on device-resident fields, by HIP events."""
    lib, stream = _hip.grf_lib(), _hip.stream_ptr(dev)
    shape = geos.r.shape
    ngeo, n = shape[-1], geos.r.size // shape[-1]
    up = lambda v, shp: torch.as_tensor(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), shp)), device=dev)
    t = {k: up(geos[k], shape) for k in POINT_FIELDS}
    t.update({k: up(geos[k], shape[:-1]) for k in RAY_FIELDS})
    Om = up(Omega, shape)
    rec = _hip.bhn_grf_geos(n, ngeo, *[t[k].data_ptr() for k in POINT_FIELDS + RAY_FIELDS], float(geos.spin), float(geos.M), float(geos.E),
                            float(geos.inc))
    nbytes = int(lib.bhn_grf_ws_bytes(n, ngeo))
    g = torch.empty(shape, dtype=torch.float64, device=dev)
    b = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
    J = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

    def calls():
        _hip.grf_check(lib.bhn_grf_doppler(C.byref(rec), _hip.ptr(Om), 0.0, 1, _hip.ptr(g), stream))
        _hip.grf_check(lib.bhn_grf_fluid_field(C.byref(rec), _hip.ptr(Om), CONSTS['arad'], CONSTS['avert'], CONSTS['ator'], _hip.ptr(b), stream))
        _hip.grf_check(lib.bhn_grf_domain_mean(C.byref(rec), _hip.ptr(b), domain[0], domain[1], domain[2], _hip.ptr(mean), _hip.ptr(ws), nbytes, stream))
        _hip.grf_check(lib.bhn_grf_transport(C.byref(rec), _hip.ptr(Om), _hip.ptr(g), _hip.ptr(b), _hip.ptr(mean), 0.85, 0.0, 1.0, _hip.ptr(J), stream))

    calls()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gr_factors_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a HIP device is needed'
    dev = torch.device('cuda:0')
    domain = (4.0, float(constants.isco_pro(SPIN)), FOV / 2.0)
    lines = ['kgeo.emission_factors: Doppler factor g and transport factors J (I, Q, U) of one hypothesis, spin %g, 60 deg, domain %s'
             % (SPIN, (domain,)), 'device: %s' % torch.cuda.get_device_name(dev), '']
    for na, ngeo in ((64, 100), (128, 64)):
        geos = kgeo.image_plane_geos(SPIN, INC, (-FOV / 2, FOV / 2), (-FOV / 2, FOV / 2), ngeo=ngeo, num_alpha=na, num_beta=na, backend='hip',
                                     device=dev).fillna(0.0)
        Omega = np.sqrt(geos.M) / (geos.r ** 1.5 + geos.spin * np.sqrt(geos.M))
        kw = dict(b_consts=CONSTS, domain=domain, Q_frac=0.85, V_frac=0)
        with np.errstate(all='ignore'):
            t_np, all_np = wall(lambda: kgeo.emission_factors(geos, Omega, **kw), 3)
        kgeo.emission_factors(geos, Omega, backend='hip', device=dev, **kw)                 # warm-up: library load, allocator
        t_hip, all_hip = wall(lambda: kgeo.emission_factors(geos, Omega, backend='hip', device=dev, **kw), 5)
        t_lib, all_lib = library_calls_ms(geos, Omega, domain, dev)
        mb_up = 8e-6 * (9 * geos.r.size + 3 * geos.alpha.size)
        mb_down = 8e-6 * 4 * geos.r.size
        lines += ['%d x %d rays x %d samples = %d points (upload %.1f MB, download %.1f MB)' % (na, na, ngeo, geos.r.size, mb_up, mb_down),
                  '  numpy   wall  %8.1f ms   (median of 3: %s)' % (1e3 * t_np, ', '.join('%.1f' % (1e3 * v) for v in all_np)),
                  '  hip     wall  %8.2f ms   (median of 5 after a warm-up, transfers included: %s)'
                  % (1e3 * t_hip, ', '.join('%.2f' % (1e3 * v) for v in all_hip)),
                  '  hip     calls %8.3f ms   (the four library calls alone, HIP events, median of 5: %s)'
                  % (t_lib, ', '.join('%.3f' % v for v in all_lib)),
                  '  numpy / hip wall: %.0fx;  share of the hip wall time outside the kernels: %.0f %%'
                  % (t_np / t_hip, 100.0 * (1.0 - 1e-3 * t_lib / t_hip)), '']
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
