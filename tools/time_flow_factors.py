#!/usr/bin/env python3
"""Time kgeo.emission_factors with a boosted-ZAMO flow (the per-setting work of the polarised-ring study: zamo_frame_velocity ->
doppler_factor -> magnetic_field_spherical -> parallel_transport) on both back ends, in one process, and write
profiles/flow_factors_time.txt.

    python tools/time_flow_factors.py [--out profiles/flow_factors_time.txt]

The study's shape: 360 rays (a circle of radius 6 on the screen) x 1000 samples, traced on the GPU, spin 0.94, 60 deg, one
(beta, chi) = (0.5, -pi / 2) setting, field (b_r, b_th, b_ph) = (0.87, 0, 0.5), V_frac = 0, in the fluid tetrad and in the ZAMO tetrad.
'numpy' is the wall time of the composed host functions (median of 3); 'hip' the wall time of the same call with backend='hip' after a
warm-up (median of 5; upload of the fields and of the field array and download of g and J included), and the three library calls alone
(zamo_velocity, doppler, transport) between two HIP events on buffers already on the device (median of 5).  No threshold: figures
only."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bhnerf_amd import _hip, kgeo                                    # noqa: E402

SPIN, INC, RHO, RAYS, NGEO = 0.94, np.deg2rad(60.0), 6.0, 360, 1000
BETA, CHI = 0.5, -np.pi / 2
FIELD = dict(b_r=0.87, b_th=0.0, b_ph=0.5)
POINT_FIELDS = ('r', 'theta', 'affine', 'Delta', 'Sigma', 'Xi', 'R', 'Theta')
RAY_FIELDS = ('lam', 'alpha', 'beta')


def wall(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def library_calls_ms(geos, zamo_frame, dev, repeats=5):
    """The three library calls alone (zamo_velocity, doppler, transport in the chosen tetrad) on device-resident buffers, by HIP events."""
    lib, stream = _hip.flow_lib(), _hip.stream_ptr(dev)
    shape = geos.r.shape
    ngeo, n = shape[-1], geos.r.size // shape[-1]
    up = lambda v, shp: torch.as_tensor(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), shp)), device=dev)
    t = {k: up(geos[k], shape) for k in POINT_FIELDS + ('omega',)}
    t.update({k: up(geos[k], shape[:-1]) for k in RAY_FIELDS})
    rec = _hip.bhn_flow_geos(n, ngeo, *[t[k].data_ptr() for k in POINT_FIELDS + RAY_FIELDS], float(geos.spin), float(geos.M), float(geos.E),
                             float(geos.inc), t['omega'].data_ptr())
    umu = torch.empty(shape + (4,), dtype=torch.float64, device=dev)
    g = torch.empty(shape, dtype=torch.float64, device=dev)
    b = up(kgeo.magnetic_field_spherical(geos, **FIELD), shape + (3,))
    J = torch.empty((3,) + shape, dtype=torch.float64, device=dev)

    def calls():
        _hip.flow_check(lib.bhn_flow_zamo_velocity(C.byref(rec), BETA, CHI, _hip.ptr(umu), stream))
        _hip.flow_check(lib.bhn_flow_doppler(C.byref(rec), _hip.ptr(umu), 0.0, 1, _hip.ptr(g), stream))
        if zamo_frame:
            _hip.flow_check(lib.bhn_flow_transport_zamo(C.byref(rec), BETA, CHI, _hip.ptr(g), _hip.ptr(b), None, 0.2, 1.0, _hip.ptr(J), stream))
        else:
            _hip.flow_check(lib.bhn_flow_transport(C.byref(rec), _hip.ptr(umu), _hip.ptr(g), _hip.ptr(b), None, 0.2, 0.0, 1.0, _hip.ptr(J), stream))

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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_factors_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a HIP device is needed'
    dev = torch.device('cuda:0')
    varphis = np.deg2rad(np.arange(RAYS) * (360.0 / RAYS) + 0.5)
    geos = kgeo.ray_geos(SPIN, INC, RHO * np.cos(varphis), RHO * np.sin(varphis), ngeo=NGEO, backend='hip', device=dev).fillna(0.0)
    mb_up = 8e-6 * (9 * geos.r.size + 3 * geos.alpha.size + 3 * geos.r.size)
    mb_down = 8e-6 * 4 * geos.r.size
    lines = ['kgeo.emission_factors(flow=(\'zamo\', %g, %.4f), b_consts=%s, V_frac=0): g and J (I, Q, U) of one setting of the ring study, '
             'spin %g, 60 deg' % (BETA, CHI, FIELD, SPIN), 'device: %s' % torch.cuda.get_device_name(dev),
             '%d rays x %d samples = %d points (upload %.1f MB, download %.1f MB)' % (RAYS, NGEO, geos.r.size, mb_up, mb_down), '']
    for frame in ('fluid', 'zamo'):
        kw = dict(flow=('zamo', BETA, CHI), b_consts=FIELD, V_frac=0, frame=frame)
        with np.errstate(all='ignore'):
            t_np, all_np = wall(lambda: kgeo.emission_factors(geos, **kw), 3)
        kgeo.emission_factors(geos, backend='hip', device=dev, **kw)                        # warm-up: library load, allocator
        t_hip, all_hip = wall(lambda: kgeo.emission_factors(geos, backend='hip', device=dev, **kw), 5)
        t_lib, all_lib = library_calls_ms(geos, frame == 'zamo', dev)
        lines += ["frame='%s'" % frame,
                  '  numpy   wall  %8.1f ms   (median of 3: %s)' % (1e3 * t_np, ', '.join('%.1f' % (1e3 * v) for v in all_np)),
                  '  hip     wall  %8.2f ms   (median of 5 after a warm-up, transfers included: %s)'
                  % (1e3 * t_hip, ', '.join('%.2f' % (1e3 * v) for v in all_hip)),
                  '  hip     calls %8.3f ms   (the three library calls alone, HIP events, median of 5: %s)'
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
