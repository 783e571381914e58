#!/usr/bin/env python3
"""Time the front end of a polarised fit -- alma.get_raytracing_args plus the first NeRF_Predictor.geometry on its result -- on the
fastest non-resident path (tracer='hip', factors='hip') and with params['resident'] = True, in one process, and write
profiles/resident_geometry_time.txt.

    timeout -k 10 600 python tools/time_resident.py [--out profiles/resident_geometry_time.txt]

Per ray set (64 x 64 rays x 100 samples and 128 x 128 x 64, spin 0.94, 60 deg, ccw Keplerian, vertical field): the wall time of both
paths after a warm-up (median of 5, the device synchronised at the end of each run), the bytes each path copies between host and
device (counted from the code, see copied_bytes), and the calls of libbhnerf_rec.so alone (bhn_rec_build, bhn_rec_kepler) between two
HIP events on samples already on the device (median of 5).  No threshold: figures only."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bhnerf_amd import _hip, alma, geodesics, network                 # noqa: E402

SPIN, INC, FOV = 0.94, np.deg2rad(60.0), 40.0
PARAMS = dict(fov_M=FOV, z_width=4.0, rmin='ISCO', Q_frac=0.85, b_consts=dict(arad=0.0, avert=1.0, ator=0.0), Omega_dir='ccw', t_start_obs=9.3,
              tracer='hip', factors='hip')


def copied_bytes(n, P, resident):
    """(host -> device, device -> host) bytes of one hypothesis of n rays and P = n * ngeo points, one chunk, counted from the code.
    Non-resident: the tracer takes alpha, beta (2n float64) and returns end and samples (7n + 7P); emission_factors uploads 8 point
    fields, Omega and 3 ray fields (9P + 3n) in image_plane_model and again in raytracing_args, and returns g, J (4P) and g (P);
    RayGeometry uploads 11 float32 planes (coords 3, Omega, J 3, g, dtau, Sigma, t_geos).  Resident: alpha, beta for the tracer, lam,
    eta for bhn_rec_build and the record's alpha, beta, lam, eta (8n float64) go up, the tracer's status check (one byte) comes down."""
    if resident:
        return 8 * 8 * n, 1
    return 8 * (2 * n + 2 * (9 * P + 3 * n)) + 4 * 11 * P, 8 * (7 * n + 7 * P + 4 * P + P) + 1


def front_end(params, pred, dev):
    rt = alma.get_raytracing_args(INC, SPIN, params)[0]
    pred.clear_geometry_cache()
    geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], rt['J'], rt['g'], rt['dtau'], rt['Sigma'])
    torch.cuda.synchronize(dev)
    return geom


def wall(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def library_calls_ms(na, ngeo, dev, repeats=5):
    """bhn_rec_build and bhn_rec_kepler alone on the device tracer's samples, by HIP events."""
    lib, stream = _hip.rec_lib(), _hip.stream_ptr(dev)
    ab = np.linspace(-FOV / 2, FOV / 2, na)
    alpha, beta = np.meshgrid(ab, ab, indexing='ij')
    beta = np.where(beta == 0.0, 1e-9, beta)
    _, samples, lam, eta, _ = geodesics._trace_device(alpha.ravel(), beta.ravel(), SPIN, INC, 1000.0, 1.0, 0.02, 5.0, 400000, ngeo, dev)
    n = alpha.size
    lam_d, eta_d = torch.as_tensor(lam, device=dev), torch.as_tensor(eta, device=dev)
    f = {k: torch.empty((n, ngeo), dtype=torch.float64, device=dev) for k in _hip.REC_FIELDS}
    Omega = torch.empty((n, ngeo), dtype=torch.float64, device=dev)
    out = _hip.bhn_rec_fields(*[f[k].data_ptr() for k in _hip.REC_FIELDS])

    def calls():
        _hip.rec_check(lib.bhn_rec_build(_hip.ptr(samples), _hip.ptr(lam_d), _hip.ptr(eta_d), n, ngeo, SPIN, 1.0, C.byref(out), stream))
        _hip.rec_check(lib.bhn_rec_kepler(_hip.ptr(f['r']), n * ngeo, SPIN, 1.0, 1.0, _hip.ptr(Omega), stream))

    calls()
    torch.cuda.synchronize(dev)
    res = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1))
    return float(np.median(res)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resident_geometry_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a HIP device is needed'
    dev = torch.device('cuda:0')
    lines = ['alma.get_raytracing_args + the first NeRF_Predictor.geometry of one hypothesis (I, Q, U), spin %g, 60 deg, fov %g M' % (SPIN, FOV),
             'device: %s' % torch.cuda.get_device_name(dev), '']
    pred = network.NeRF_Predictor(FOV / 2, 2.0, FOV / 2, 4.0, net_depth=4, net_width=128, device=dev)
    for na, ngeo in ((64, 100), (128, 64)):
        n, P = na * na, na * na * ngeo
        rows = {}
        for label, resident in (('hip', False), ('resident', True)):
            params = dict(PARAMS, num_alpha=na, num_beta=na, resident=resident)
            # a tracer call holds `chunk` rays: geodesics' default (65536) takes both ray sets whole
            front_end(params, pred, dev)                                                    # warm-up: library load, allocator
            rows[label] = wall(lambda: front_end(params, pred, dev), 5) + copied_bytes(n, P, resident)
        t_lib, all_lib = library_calls_ms(na, ngeo, dev)
        lines.append('%d x %d rays x %d samples = %d points' % (na, na, ngeo, P))
        for label, (t, every, up, down) in rows.items():
            lines.append('  %-9s wall %8.2f ms   (median of 5 after a warm-up: %s);  host -> device %.2f MB, device -> host %.2f MB'
                         % (label, 1e3 * t, ', '.join('%.2f' % (1e3 * v) for v in every), 1e-6 * up, 1e-6 * down))
        lines += ['  rec calls      %8.3f ms   (bhn_rec_build + bhn_rec_kepler alone, HIP events, median of 5: %s)'
                  % (t_lib, ', '.join('%.3f' % v for v in all_lib)),
                  '  hip / resident wall: %.2fx' % (rows['hip'][0] / rows['resident'][0]), '']
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
