#!/usr/bin/env python3
"""Time the EHT chi-square from (u, v) coordinates (libbhnerf_eht.so, observation.DirectDFT) against the dense-matrix path
(bhn_chi2_eht) on the device, in one process:

  config-4 shape   8 frames x 28 baselines x 256 x 256 pixels, 'vis' loss + image gradient: dense engine.chi2_eht and the
                   matrix-free path, 3 warm-ups, median of 10 event-timed calls each; the time to build and upload each operator
                   (dense: observation.dft_matrix on the host + the copy; matrix-free: the copy of uv) separately
  20-station shape 190 baselines, 1140 triangles, 8 frames, 'vis' and 'cphase' on the matrix-free path only, with the bytes a
                   dense A would need beside it

Writes profiles/eht_uv_time.txt (or --out) and exits non-zero unless the matrix-free median of the config-4 shape is no larger
than the dense one.

  python tools/time_eht_uv.py [--out profiles/eht_uv_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bhnerf_amd import _hip, engine, observation        # noqa: E402

RAD_PER_M = 5.03e-6 / 3600.0 * np.pi / 180.0
FOV = 16.0 * RAD_PER_M
NPIX, NT = 256, 8


def median_ms(fn, warmup=3, calls=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def array(ns, rng):
    pos = rng.normal(size=(NT, ns, 2)) * 3e9
    pairs = np.array([(i, j) for i in range(ns) for j in range(i + 1, ns)])
    return np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]]), pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eht_uv_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(NPIX) - 127.5, np.arange(NPIX) - 127.5, indexing='ij')
    img = np.exp(-0.5 * (yy ** 2 + xx ** 2) / 12.0 ** 2)[None] + 0.05 * rng.uniform(size=(NT, NPIX, NPIX))
    images = torch.as_tensor((img * (2.0 / img.sum(axis=(1, 2), keepdims=True))).astype(np.float32), device=dev)
    flat = images.reshape(NT, -1)
    lines = ['EHT chi-square + image gradient per call, %d frames x %d x %d pixels, median of 10 event-timed calls after 3 warm-ups (%s)'
             % (NT, NPIX, NPIX, torch.cuda.get_device_name(0))]

    # ---- config-4 shape: 28 baselines, 'vis'
    uv, _ = array(8, rng)
    nvis = uv.shape[1]
    target = (rng.normal(size=(NT, nvis)) + 1j * rng.normal(size=(NT, nvis))).astype(np.complex64)
    sigma = np.full((NT, nvis), 0.1, dtype=np.float32)
    tgt, sig = torch.as_tensor(target, device=dev), torch.as_tensor(sigma, device=dev)
    t0 = time.perf_counter()
    A_host = np.stack([observation.dft_matrix(u, FOV, NPIX) for u in uv])
    t1 = time.perf_counter()
    A = torch.as_tensor(A_host, device=dev)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    op = observation.DirectDFT(uv, FOV, NPIX).to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    dense_ms = median_ms(lambda: engine.chi2_eht(flat, A, tgt, sig, 1.0, 'vis'))
    uv_ms = median_ms(lambda: engine.chi2_eht(images, op, tgt, sig, 1.0, 'vis'))
    # the library calls alone, every buffer allocated once: what the device does, without the Python around it
    lib, elib, st = _hip.lib(), _hip.eht_lib(), _hip.stream_ptr(dev)
    R = NPIX * NPIX
    Ar, tr = torch.view_as_real(A), torch.view_as_real(tgt)
    wsd = torch.empty((int(lib.bhn_chi2_eht_ws_floats(NT, 1, nvis, R)),), dtype=torch.float32, device=dev)
    nb = int(elib.bhn_eht_ws_bytes(NT, nvis, 0, NPIX, NPIX))
    wsu = torch.empty((nb,), dtype=torch.uint8, device=dev)
    loss1, dimg1 = torch.empty((1,), dtype=torch.float32, device=dev), torch.empty_like(images)
    psize = FOV / NPIX
    dense_lib_ms = median_ms(lambda: _hip.check(lib.bhn_chi2_eht(_hip.ptr(flat), _hip.ptr(Ar), _hip.ptr(tr), _hip.ptr(sig), 1.0, 0, NT, 1, nvis, R,
                                                                  _hip.ptr(wsd), _hip.ptr(loss1), _hip.ptr(dimg1), st)))
    uv_lib_ms = median_ms(lambda: _hip.eht_check(elib.bhn_eht_chi2_uv(_hip.ptr(images), _hip.ptr(op.uv), NT, 1, nvis, NPIX, NPIX, psize, psize, 0, _hip.ptr(tr),
                                                                      _hip.ptr(sig), 1.0, None, None, 0, _hip.ptr(loss1), _hip.ptr(dimg1), _hip.ptr(wsu), nb, st)))
    ld, gd = engine.chi2_eht(flat, A, tgt, sig, 1.0, 'vis')
    lu, gu = engine.chi2_eht(images, op, tgt, sig, 1.0, 'vis')
    ws = int(_hip.eht_lib().bhn_eht_ws_bytes(NT, nvis, 0, NPIX, NPIX))
    img_bytes = NT * NPIX * NPIX * 4
    kb = (nvis + 7) // 8
    lines += [
        'config-4 shape, %d baselines, vis:' % nvis,
        '  dense        %.3f ms per call   operator: %.3f s on the host + %.3f s upload, %.1f MB resident per %d frames; A streamed twice: %.1f MB per call'
        % (dense_ms, t1 - t0, t2 - t1, A_host.nbytes / 1e6, NT, 2 * A_host.nbytes / 1e6),
        '  matrix-free  %.3f ms per call   operator: %.6f s (copy of uv), %.4f MB resident per %d frames; workspace %.2f MB; the images are read %d times (from L2 after the first) and '
        'dimages written once (%.1f MB) plus the tables (%.2f MB) -- counted, not measured'
        % (uv_ms, t3 - t2, uv.nbytes / 1e6, NT, ws / 1e6, kb, (kb + 1) * img_bytes / 1e6, NT * nvis * 2 * NPIX * 8 * 2 / 1e6),
        '  the library calls alone (buffers allocated once): dense %.3f ms, matrix-free %.3f ms' % (dense_lib_ms, uv_lib_ms),
        '  loss dense %.6e matrix-free %.6e (relative difference %.1e); dimages max difference / max %.1e'
        % (ld.item(), lu.item(), abs(ld.item() - lu.item()) / abs(ld.item()), float((gd.reshape(gu.shape) - gu).abs().max() / gd.abs().max())),
    ]
    del A, Ar, gd, gu

    # ---- 20-station shape: 190 baselines, 1140 triangles, matrix-free only
    uv, pairs = array(20, rng)
    nvis = uv.shape[1]
    triangles = observation.closure_triangles(20)
    ncp = len(triangles)
    lines.append('20-station shape, %d baselines, %d triangles, matrix-free only:' % (nvis, ncp))
    for dtype in ('vis', 'cphase'):
        op = (observation.DirectDFT(uv, FOV, NPIX, triangles=triangles, pairs=pairs) if dtype == 'cphase' else observation.DirectDFT(uv, FOV, NPIX)).to(dev)
        n = ncp if dtype == 'cphase' else nvis
        tgt = torch.as_tensor((rng.normal(size=(NT, n)) + 1j * rng.normal(size=(NT, n))).astype(np.complex64) if dtype == 'vis'
                              else rng.uniform(-3, 3, (NT, n)).astype(np.float32), device=dev)
        sig = torch.full((NT, n), 0.1, dtype=torch.float32, device=dev)
        ms = median_ms(lambda: engine.chi2_eht(images, op, tgt, sig, 1.0, dtype))
        rows = (3 * ncp if dtype == 'cphase' else nvis)
        lines.append('  %-6s %.3f ms per call; workspace %.2f MB; a dense A would hold %.2f GB per %d frames (%.1f GB for 64 frames) -- computed, not allocated'
                     % (dtype, ms, int(_hip.eht_lib().bhn_eht_ws_bytes(NT, nvis, op.ncp, NPIX, NPIX)) / 1e6, NT * rows * NPIX * NPIX * 8 / 1e9, NT,
                        64 * rows * NPIX * NPIX * 8 / 1e9))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    if not uv_ms <= dense_ms:
        print('FAIL: the matrix-free median (%.3f ms) is larger than the dense one (%.3f ms)' % (uv_ms, dense_ms))
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
