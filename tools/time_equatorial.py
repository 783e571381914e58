"""Time the equatorial crossings and the lensing inverse built on them, both back ends in one process on the same box.

    python tools/time_equatorial.py [--out profiles/equatorial_time.txt] [--reps 5]

Lines written (one JSON object each):
  crossings   geodesics.equatorial_crossings at 64 x 64 rays over (-8, 8)^2, spin 0.94, inclination 60 deg, nmax = 3:
              numpy_s   wall time of backend='numpy'
              hip_s     wall time of backend='hip' after one warm-up call (upload, kernel, download), median of --reps
              kernel_ms the kernel alone: HIP events around bhn_eql_crossings on device buffers, median of --reps (and the least)
              steps     step count of the slowest lane (the kernel's `status`)
              max_row_diff  largest difference of a row between the back ends, relative to the row's largest magnitude
  rho_of_req  one kgeo.equatorial_lensing.rho_of_req call, 64 angles, req = 6, mbar 0, 1 and 2, backend='hip' (wall time, the number
              of crossings calls it made); at mbar 0 also backend='numpy'
No ratio is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPIN, INC, SIDE, NMAX, FOV = 0.94, np.deg2rad(60.0), 64, 3, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'equatorial_time.txt'))
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    from bhnerf_amd import _hip, geodesics as G, kgeo
    dev = torch.device('cuda:0')
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    alpha, beta = np.meshgrid(np.linspace(-FOV, FOV, SIDE), np.linspace(-FOV, FOV, SIDE), indexing='ij')
    alpha, beta = alpha.ravel(), np.where(beta == 0.0, 1e-9, beta).ravel()
    n = alpha.size
    t0 = time.perf_counter()
    host = G.equatorial_crossings(alpha, beta, SPIN, INC, nmax=NMAX)
    numpy_s = time.perf_counter() - t0
    got = G.equatorial_crossings(alpha, beta, SPIN, INC, nmax=NMAX, backend='hip', device=dev)       # warm-up: library load, first launch
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = G.equatorial_crossings(alpha, beta, SPIN, INC, nmax=NMAX, backend='hip', device=dev)
        walls.append(time.perf_counter() - t0)
    same_count = bool(np.array_equal(got.count, host.count))
    diff = 0.0
    for k in ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth'):
        both = np.isfinite(got[k]) & np.isfinite(host[k])
        diff = max(diff, float(np.abs(got[k][both] - host[k][both]).max() / np.abs(host[k][both]).max()))
    a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
    cross = torch.empty((7, n, NMAX), dtype=torch.float64, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    times = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.eql_check(_hip.eql_lib().bhn_eql_crossings(_hip.ptr(a_d), _hip.ptr(b_d), n, SPIN, INC, 1000.0, 1.0, 0.02, 5.0, 400000, NMAX,
                                                        _hip.ptr(cross), _hip.ptr(count), _hip.ptr(status), _hip.stream_ptr(dev)))
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
    times = times[1:]
    st = status.cpu().numpy()
    assert (st > 0).all()
    emit(what='crossings', spin=SPIN, inclination_deg=60.0, rays=n, nmax=NMAX, crossings=int(host.count.sum()), numpy_s=round(numpy_s, 3),
         hip_s=round(float(np.median(walls)), 4), kernel_ms=round(float(np.median(times)), 3), kernel_min_ms=round(min(times), 3),
         steps=int(st.max()), numpy_over_hip=round(numpy_s / float(np.median(walls)), 1), same_count=same_count, max_row_diff=diff)

    varphis = np.linspace(-np.pi, np.pi, 64, endpoint=False)
    calls = [0]
    traced = G.equatorial_crossings

    def counting(*a, **kw):
        calls[0] += 1
        return traced(*a, **kw)

    G.equatorial_crossings = counting
    try:
        for mbar, backends in ((0, ('hip', 'numpy')), (1, ('hip',)), (2, ('hip',))):
            for backend in backends:
                calls[0] = 0
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rho = kgeo.equatorial_lensing.rho_of_req(SPIN, INC, 6.0, mbar=mbar, varphis=varphis, backend=backend, device=dev)[0]
                emit(what='rho_of_req', backend=backend, mbar=mbar, angles=64, req=6.0, seconds=round(time.perf_counter() - t0, 3),
                     crossings_calls=calls[0], rho_min=float(rho.min()), rho_max=float(rho.max()))
    finally:
        G.equatorial_crossings = traced
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
