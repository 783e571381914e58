"""Time geodesics.image_plane_geos with both back ends on the same box: the NumPy tracer on the host against bhn_kerr_trace
(csrc/kerr_trace.hip) on the GPU.

    python tools/time_tracer.py                 # both shapes, each in a child process under its own time limit
    python tools/time_tracer.py --one config5   # one shape, in this process

Shapes: `config5` 64 x 64 rays x 100 samples, spin 0, inclination 12 deg, field of view 40 M (BASELINE config 5, the ALMA fit);
`config2` 128 x 128 x 64, spin 0.5, 60 deg, 16 M (BASELINE config 2).  Per shape one JSON line:
  numpy_s     wall time of image_plane_geos(backend='numpy') -- the baseline: the code every caller ran before the device tracer
  hip_s       wall time of image_plane_geos(backend='hip') after one warm-up call (upload, kernel, download, the shared NumPy
              post-processing that builds the record), median of --reps
  kernel_ms   the kernel alone: HIP events around bhn_kerr_trace on device buffers, median of --reps (and the least)
  steps       first-pass step count of the slowest ray (the kernel's `status`): what sets the time of both back ends
  max_row_diff  largest difference of a sampled row between the back ends, relative to the row's largest magnitude
The script fails unless the hip back end is faster than the numpy one at the shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {        # name -> (spin, inclination [deg], rays per side, samples per ray, field of view [M])
    'config5': (0.0, 12.0, 64, 100, 40.0),
    'config2': (0.5, 60.0, 128, 64, 16.0),
}


def one(name, reps):
    import torch
    from bhnerf_amd import _hip, geodesics as G
    spin, inc_deg, side, ngeo, fov = SHAPES[name]
    inc = np.deg2rad(inc_deg)
    args = (spin, inc, (-fov / 2, fov / 2), (-fov / 2, fov / 2))
    kw = dict(ngeo=ngeo, num_alpha=side, num_beta=side)
    dev = torch.device('cuda:0')
    t0 = time.perf_counter()
    host = G.image_plane_geos(*args, backend='numpy', **kw)
    numpy_s = time.perf_counter() - t0
    got = G.image_plane_geos(*args, backend='hip', device=dev, **kw)           # warm-up: library load, first launch
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = G.image_plane_geos(*args, backend='hip', device=dev, **kw)
        walls.append(time.perf_counter() - t0)
    diff = max(float(np.abs(got[k] - host[k]).max() / np.abs(host[k]).max()) for k in G.SAMPLE_ROWS)
    # the kernel alone, through the ABI on prepared device buffers
    n = side * side
    beta = np.where(host.beta == 0.0, 1e-9, host.beta)
    a_d, b_d = torch.as_tensor(host.alpha.ravel(), device=dev), torch.as_tensor(beta.ravel(), device=dev)
    end = torch.empty((7, n), dtype=torch.float64, device=dev)
    samples = torch.empty((7, n, ngeo), dtype=torch.float64, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.kerr_check(_hip.kerr_lib().bhn_kerr_trace(_hip.ptr(a_d), _hip.ptr(b_d), n, spin, inc, 1000.0, 1.0, 0.02, 5.0, 400000, ngeo, _hip.ptr(samples),
                                             _hip.ptr(end), _hip.ptr(status), _hip.stream_ptr(dev)))
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
    times = times[1:]
    st = status.cpu().numpy()
    assert (st > 0).all()
    assert samples[1].cpu().numpy().tobytes() == np.ascontiguousarray(got.r.reshape(n, ngeo)).tobytes()         # the same kernel, the same bytes
    hip_s = float(np.median(walls))
    out = dict(shape=name, spin=spin, inclination_deg=inc_deg, rays=n, samples_per_ray=ngeo, fov_M=fov, numpy_s=round(numpy_s, 3),
               hip_s=round(hip_s, 4), kernel_ms=round(float(np.median(times)), 3), kernel_min_ms=round(min(times), 3),
               steps=int(st.max()), us_per_step=round(1e3 * float(np.median(times)) / (2 * int(st.max())), 3),
               numpy_over_hip=round(numpy_s / hip_s, 1), max_row_diff=diff)
    print(json.dumps(out), flush=True)
    if not hip_s < numpy_s:
        sys.exit('%s: the hip back end (%.3f s) is not faster than the numpy back end (%.3f s)' % (name, hip_s, numpy_s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', choices=list(SHAPES))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=400, help='seconds per shape')
    args = ap.parse_args()
    if args.one:
        one(args.one, args.reps)
        return
    for name in SHAPES:                                              # a fresh child per shape, each under its own time limit
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', name, '--reps', str(args.reps)], timeout=args.limit)
        if res.returncode != 0:
            sys.exit('shape %s failed with exit status %d: stopping' % (name, res.returncode))


if __name__ == '__main__':
    main()
