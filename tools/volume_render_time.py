"""Time VolumeVisualizer.render (bhn_volume_render, csrc/volume_render.hip) at 64^3 and 256^3 with the wireframe and the black hole.

    python tools/volume_render_time.py            # both sizes, each in a child process under its own time limit
    python tools/volume_render_time.py --one 64   # one size, in this process

Per size: device-event time of one render after a warm-up (median of --reps), the number of wireframe terms the kernel's culling
keeps (counted on the host by the kernel's own rules, before its early exit at alpha >= 1: an upper bound of the exp it evaluates)
against the 3072 per point of the reference, and the exp rate that implies against the v_exp_f32 issue rate of the
MI355X (8 cycles per 64-lane instruction per SIMD: 256 CUs x 4 SIMDs x 8 lanes / cycle at 2.4 GHz = 1.97e13 / s).
A record for DESIGN.md, not a gate: there is no earlier implementation to compare against.
"""
import argparse
import json
import subprocess
import sys
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXP_PEAK = 256 * 4 * 8 * 2.4e9
CAM_R, DOMAIN_R, LINEWIDTH, BH_RADIUS = 37.0, 8.0, 0.1, 2.0
FACEWIDTH = 1.9 * DOMAIN_R


def kept_terms(pts, fw, lw, bh):
    """(points that reach the wireframe sum, points past its pre-test, terms kept by the segment and range tests)."""
    h, cut = fw / 2, 39.0 * lw * lw
    step = fw / 63.0
    reach = past = terms = 0
    for row in pts:                                                    # (W, S, 3) at a time
        p = row.reshape(-1, 3).astype(np.float64)
        live = (np.abs(p).max(-1) <= h + lw) & ~((p ** 2).sum(-1) < bh * bh)
        p = p[live]
        reach += len(p)
        p = p[(np.abs(np.abs(p) - h) <= cut).sum(-1) >= 2]
        past += len(p)
        for i in range(8):
            u = p - np.array([h if i & 1 else -h, h if i & 2 else -h, h if i & 4 else -h])
            for j in range(6):
                c = j // 2
                r2 = u[:, (c + 1) % 3] ** 2 + u[:, (c + 2) % 3] ** 2
                along = u[:, c] if j & 1 else -u[:, c]
                lo, hi = np.maximum((along - cut) / step, 0.0), np.minimum((along + cut) / step, 63.0)
                ok = (r2 <= cut * cut) & (lo <= hi)
                terms += int((np.ceil(hi[ok]) - np.floor(lo[ok]) + 1).sum())
    return reach, past, terms


def one(size, reps):
    import torch
    from bhnerf_amd import visualization
    viz = visualization.VolumeVisualizer(size, size, size)
    viz.set_view(CAM_R, DOMAIN_R, 0.6, 1.1)
    x, y, z = viz.x, viz.y, viz.z
    e = np.exp(-((x - 4.0) ** 2 + (y + 1.0) ** 2 + (z - 0.5) ** 2) / (2 * 1.3 ** 2)).astype(np.float32)
    dev = torch.device('cuda:0')
    em = torch.as_tensor(e, device=dev)
    kw = dict(bh_radius=BH_RADIUS, linewidth=LINEWIDTH, bh_albedo=[0.5, 0.5, 0.5], cmap=np.linspace(0, 1, 768).reshape(256, 3))
    img = viz.render(em, FACEWIDTH, **kw)                               # warm-up: device copy of the points, first launch
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        img = viz.render(em, FACEWIDTH, **kw)
        t1.record()
        torch.cuda.synchronize(dev)
        times.append(t0.elapsed_time(t1))
    render_ms = float(np.median(times))
    # the kernel alone, through the ABI on prepared device buffers
    import ctypes as C
    from bhnerf_amd import _hip
    pts_dev, lut = viz._device_points(dev), torch.as_tensor(np.ascontiguousarray(kw['cmap'], dtype=np.float32), device=dev)
    scale = (1.0 / em.amax()).reshape(1).contiguous()
    images = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
    view = _hip.bhn_volume_view(FACEWIDTH, LINEWIDTH, BH_RADIUS, (C.c_double * 3)(0.5, 0.5, 0.5))
    times = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _hip.check(_hip.lib().bhn_volume_render(_hip.ptr(pts_dev), _hip.ptr(em), _hip.ptr(scale), 1, size, size, size, size ** 3, _hip.ptr(lut), 256,
                                                C.byref(view), _hip.ptr(images), _hip.stream_ptr(dev)))
        t1.record()
        torch.cuda.synchronize(dev)
        times.append(t0.elapsed_time(t1))
    times = times[1:]
    assert images.cpu().numpy().tobytes() == img.cpu().numpy().tobytes()
    ms = float(np.median(times))
    reach, past, terms = kept_terms(viz._pts.astype(np.float32), FACEWIDTH, LINEWIDTH, BH_RADIUS)
    n = size ** 3
    out = dict(size=size, python_render_ms=round(render_ms, 4), kernel_ms=round(ms, 4), kernel_min_ms=round(min(times), 4), points=n, points_reaching_wire_sum=reach, points_past_pretest=past,
               terms_kept=terms, terms_reference=3072 * n, kept_fraction=terms / (3072.0 * n), exp_per_s=terms / (ms * 1e-3),
               exp_rate_of_peak=terms / (ms * 1e-3) / EXP_PEAK, reference_exp_per_s_equivalent=3072.0 * n / (ms * 1e-3),
               image_min=float(img.min()), image_max=float(img.max()))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--one', type=int, default=0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--limit', type=int, default=240, help='seconds per size')
    args = ap.parse_args()
    if args.one:
        one(args.one, args.reps)
        return
    for size in (64, 256):                                             # a fresh child per size, each under its own time limit
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', str(size), '--reps', str(args.reps)], timeout=args.limit)
        if res.returncode != 0:
            sys.exit('size %d failed with exit status %d: stopping' % (size, res.returncode))


if __name__ == '__main__':
    main()
