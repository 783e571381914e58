#!/usr/bin/env python3
"""Time the volume priors (libbhnerf_reg.so, regularization.VolumePrior) on the device, in one process:

  library    bhn_reg_loss with all three terms on one 64^3 and one 128^3 volume (a smooth hotspot on a noisy floor, the domain
             mask of a recovery: 3 <= r <= fov / 2, |z| <= 4), with and without the gradient, every buffer allocated once; the
             same call through engine.chi2_volume (buffers allocated per call, weights normalised)
  context    the same loss and gradient written with torch ops and autograd on the same device -- what a user would write
             without the library; not a reference, the tests hold the kernels to float64
  step       one TrainStep.volume_prior step (64^3 and 32^3 lattice) beside one TrainStep.image 'lc' step at BASELINE config 5's
             shape (64 x 64 rays x 100 samples, Stokes I/Q/U, 4x128 bf16, 8 frames per step), same predictor, host-timed over
             50 steps after 5 warm-ups
  bytes      what a call touches, counted from the code (csrc/vol_reg.hip)

3 warm-ups, median of 10 event-timed calls each.  Nothing is asserted on time.  Writes profiles/vol_reg_time.txt (or --out).

  python tools/time_reg.py [--out profiles/vol_reg_time.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
from bhnerf_amd import _hip, engine, network, optimization, regularization, synthetic, units        # noqa: E402
from time_eht_uv import median_ms                                                                   # noqa: E402

FOV, WEIGHTS, EPS = 20.0, {'tv': 1.0, 'tsv': 0.3, 'l1': 0.2}, 1e-3


def volume(n, rng):
    ax = np.linspace(-FOV / 2, FOV / 2, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    mask = ((r >= 3.0) & (r <= FOV / 2) & (np.abs(z) <= 4.0)).astype(np.uint8)
    e = 4.5e-5 + np.exp(-((x - 5.5) ** 2 + y ** 2 + z ** 2) / (2 * 1.5 ** 2)) + 0.01 * rng.uniform(size=x.shape)
    return (e * mask).astype(np.float32), mask


def torch_prior(e, m, h, w, eps, scale):
    """The formulas of include/bhnerf_reg.h with torch ops; the gradient by autograd."""
    e = e.detach().requires_grad_(True)
    q = torch.zeros_like(e)
    for axis in range(3):
        n = e.shape[axis]
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        d = torch.zeros_like(e)
        d[tuple(lo)] = (e[tuple(hi)] - e[tuple(lo)]) * (m[tuple(lo)] * m[tuple(hi)]) / h[axis]
        q = q + d * d
    loss = scale * (w[0] * (m * torch.sqrt(q + eps * eps)).sum() + w[1] * (m * q).sum() + w[2] * (m * e.abs()).sum())
    loss.backward()
    return loss.detach(), e.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vol_reg_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    lib, st = _hip.reg_lib(), _hip.stream_ptr(dev)
    f3 = C.c_float * 3
    lines = ['volume priors tv + tsv + l1 per call on one volume, median of 10 event-timed calls after 3 warm-ups (%s)' % torch.cuda.get_device_name(0)]
    for n in (64, 128):
        vol, mask = volume(n, rng)
        e, m = torch.as_tensor(vol, device=dev), torch.as_tensor(mask, device=dev)
        op = regularization.VolumePrior(fov=FOV, resolution=n, weights=WEIGHTS, eps=EPS)
        V, inside = n ** 3, int(mask.sum())
        nb = int(lib.bhn_reg_ws_bytes(1, n, n, n))
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        loss4, pv, dvol = torch.empty((4,), device=dev), torch.empty((3, 1), device=dev), torch.empty_like(e)
        w = f3(*op.call_weights(m))
        call = lambda grad=True: _hip.reg_check(lib.bhn_reg_loss(
            e.data_ptr(), 1, n, n, n, m.data_ptr(), f3(*op.spacing), w, EPS, 1.0, loss4.data_ptr(), pv.data_ptr(), dvol.data_ptr() if grad else None,
            ws.data_ptr(), nb, st))
        lib_ms, fwd_ms = median_ms(call), median_ms(lambda: call(False))
        eng_ms = median_ms(lambda: engine.chi2_volume(e, op, 1.0, mask=m))
        four = loss4.cpu().numpy()
        mf = m.to(torch.float32)
        wn = [v / inside for v in op.weights]
        torch_ms = median_ms(lambda: torch_prior(e, mf, op.spacing, wn, EPS, 1.0))
        tl, tg = torch_prior(e, mf, op.spacing, wn, EPS, 1.0)
        chunks = (V + 1023) // 1024
        # per voxel from memory: e (4 bytes) and the mask (1) once -- the 12 other loads of e and the neighbours' mask bytes of a voxel
        # are re-reads of lines its own or a neighbouring workgroup has brought in -- and the gradient (4); per workgroup 3 partial sums
        touched = V * (4 + 1) + chunks * 12 * 2 + 16 + 12
        lines += ['%d^3 voxels, %d in the mask (%.0f %%), workspace %d bytes' % (n, inside, 100.0 * inside / V, nb),
                  '  library call alone (buffers allocated once)   %.4f ms with the gradient, %.4f ms forward only' % (lib_ms, fwd_ms),
                  '  engine.chi2_volume (allocates per call)       %.4f ms with the gradient' % eng_ms,
                  '  the same with torch ops and autograd          %.4f ms (context, not a reference); loss %.6e, gradient differs by %.1e of its max'
                  % (torch_ms, float(tl), float((tg - dvol).abs().max() / tg.abs().max())),
                  '  loss terms {total, tv, tsv, l1} = %s' % ', '.join('%.6e' % v for v in four),
                  '  bytes touched per call, counted from the code: %.2f MB forward only, %.2f MB with the gradient (unique addresses; the kernel'
                  % (touched / 1e6, (touched + 4 * V) / 1e6),
                  '  issues 13 loads of e and up to 7 of the mask per in-mask voxel, all but the first of each served by L1 / L2):'
                  ' %.0f GB/s with the gradient' % ((touched + 4 * V) / 1e6 / lib_ms)]

    # one prior step beside one 'lc' image step at config 5's shape, same predictor and state
    c = dict(H=64, W=64, G=100, width=128, fov=40.0, inc=12.0, spin=0.0, rmin=6.0, rmax=20.0, z_width=4.0)
    geo = synthetic.synthetic_geodesics(c['H'], c['W'], c['G'], fov_M=c['fov'], inc_deg=c['inc'], spin=c['spin'], S=3, seed=3)
    nt, B = 128, 8
    t_frames = np.linspace(0.0, 1.7, nt)
    rt = network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                      t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr, J=geo['J'])
    target = np.random.default_rng(5).uniform(0.5, 1.5, (nt, 3)).astype(np.float32)
    pred = network.NeRF_Predictor(c['rmax'], c['rmin'], c['rmax'], c['z_width'], net_depth=4, net_width=c['width'], mode='bf16', device=dev)
    opt = optimization.Optimizer({'num_iters': 100000, 'lr_init': 1e-4, 'lr_final': 1e-6}, pred, rt)
    image = optimization.TrainStep.image(t_frames * units.hr, target, sigma=0.1, dtype='lc')
    frames = image.args[0]

    def steps_ms(step, count=50):
        for _ in range(5):
            _, opt.state, _ = step(opt.state, rt, frames.sample(B))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            _, opt.state, _ = step(opt.state, rt, frames.sample(B))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    lines.append("training steps at BASELINE config 5's shape (64 x 64 rays x 100 samples, I/Q/U, 4x128 bf16, %d frames per step), host-timed, 50 steps" % B)
    lines.append("  TrainStep.image 'lc' alone                           %.3f ms per step" % steps_ms(image))
    for res in (32, 64):
        prior = optimization.TrainStep.volume_prior(c['fov'], resolution=res, weights={'tv': 1.0})
        p_ms = steps_ms(prior)
        geom = pred.geometry(prior.args[0].op.coords, 0.0, 0.0)
        lines.append('  TrainStep.volume_prior alone, %3d^3 lattice           %.3f ms per step (%d of %d voxels in the domain)'
                     % (res, p_ms, int(geom.dom.sum()), res ** 3))
        lines.append("  TrainStep.image 'lc' + TrainStep.volume_prior %3d^3   %.3f ms per call (two Adam steps)" % (res, steps_ms(image + prior)))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
