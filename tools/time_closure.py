#!/usr/bin/env python3
"""Time the combined closure loss (libbhnerf_cls.so, observation.ClosureDFT, TrainStep.eht_closure) on the device, in one process:

  config-4 shape    8 frames x 256 x 256 pixels, an 8-station array: 28 baselines, 56 triangles, 140 quadrangles
  20-station shape  190 baselines, 1140 triangles, 9690 quadrangles, the same frames

For each: the library call alone for 'cphase+logcamp' (loss + image gradient, every buffer allocated once), the same call through
engine.chi2_eht, and beside them the two single-term calls of the (u, v) path it replaces ('cphase' through libbhnerf_eht.so,
'logcamp' through libbhnerf_cls.so alone).  3 warm-ups, median of 10 event-timed calls.

Then one training step at the config-4 shape (256 x 256 rays x 100 samples, 4x256 bf16, 8 frames per step): ONE combined
TrainStep.eht_closure step ('cphase+logcamp': one render, one visibility pass, one Adam step) against the TrainStep.__add__ of
the two single-term steps (two renders, two Adam steps: the reference's semantics), wall time per step, median of 5 after 2 warm-ups.

Nothing is asserted on time.  Writes profiles/closure_time.txt (or --out).

  python tools/time_closure.py [--out profiles/closure_time.txt]
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
from bhnerf_amd import _hip, engine, network, observation, optimization, synthetic, units        # noqa: E402
from time_eht_uv import FOV, NPIX, NT, array, median_ms                                          # noqa: E402


def wall_ms(fn, warmup=2, calls=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'closure_time.txt'))
    ap.add_argument('--no-step', action='store_true', help='skip the training step')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(NPIX) - 127.5, np.arange(NPIX) - 127.5, indexing='ij')
    img = np.exp(-0.5 * (yy ** 2 + xx ** 2) / 12.0 ** 2)[None] + 0.05 * rng.uniform(size=(NT, NPIX, NPIX))
    images = torch.as_tensor((img * (2.0 / img.sum(axis=(1, 2), keepdims=True))).astype(np.float32), device=dev)
    lines = ["combined closure loss 'cphase+logcamp' + image gradient per call, %d frames x %d x %d pixels, median of 10 event-timed calls after 3 warm-ups (%s)"
             % (NT, NPIX, NPIX, torch.cuda.get_device_name(0))]
    lib, st, psize = _hip.cls_lib(), _hip.stream_ptr(dev), FOV / NPIX
    kept = {}
    for ns in (8, 20):
        uv, pairs = array(ns, rng)
        nvis = uv.shape[1]
        tris, quads = observation.closure_triangles(ns), observation.closure_quadrangles(ns)
        op = observation.ClosureDFT(uv, FOV, NPIX, pairs=pairs, triangles=tris, quadrangles=quads).to(dev)
        only_q = observation.ClosureDFT(uv, FOV, NPIX, pairs=pairs, quadrangles=quads).to(dev)
        plain = observation.DirectDFT(uv, FOV, NPIX, triangles=tris, pairs=pairs).to(dev)
        ncp, nca = op.ncp, op.nca
        vis = op.observe(images).cpu().numpy()
        cp = torch.as_tensor((op.closure_phases(vis) + 0.3).astype(np.float32), device=dev)
        lca = torch.as_tensor((op.log_closure_amplitudes(vis) + 0.2).astype(np.float32), device=dev)
        scp, slca = torch.full_like(cp, 0.1), torch.full_like(lca, 0.1)
        tgt, sig = torch.cat([cp, lca], dim=-1), torch.cat([scp, slca], dim=-1)
        nb = int(lib.bhn_cls_ws_bytes(NT, nvis, ncp, nca, NPIX, NPIX))
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        loss4, dimg = torch.empty((4,), dtype=torch.float32, device=dev), torch.empty_like(images)
        tc, tq = _hip.bhn_cls_term(cp.data_ptr(), scp.data_ptr(), 1.0), _hip.bhn_cls_term(lca.data_ptr(), slca.data_ptr(), 1.0)
        call = lambda grad=True: _hip.cls_check(lib.bhn_cls_chi2(
            _hip.ptr(images), _hip.ptr(op.uv), NT, 1, nvis, NPIX, NPIX, psize, psize, None, C.byref(tc), C.byref(tq), _hip.ptr(op.tri),
            _hip.ptr(op.tri_sign), ncp, _hip.ptr(op.quad), nca, 1.0, _hip.ptr(loss4), _hip.ptr(dimg) if grad else None, _hip.ptr(ws), nb, st))
        lib_ms, fwd_ms = median_ms(call), median_ms(lambda: call(False))
        eng_ms = median_ms(lambda: engine.chi2_eht(images, op, tgt, sig, 1.0, 'cphase+logcamp'))
        cp_ms = median_ms(lambda: engine.chi2_eht(images, plain, cp, scp, 1.0, 'cphase'))
        lq_ms = median_ms(lambda: engine.chi2_eht(images, only_q, lca, slca, 1.0, 'logcamp'))
        four = op.last_terms.cpu().numpy()
        lines += ['%d stations: %d baselines, %d triangles, %d quadrangles; workspace %.2f MB' % (ns, nvis, ncp, nca, nb / 1e6),
                  '  library call alone (buffers allocated once)   %.3f ms with the gradient, %.3f ms forward only' % (lib_ms, fwd_ms),
                  "  engine.chi2_eht(.., 'cphase+logcamp')          %.3f ms" % eng_ms,
                  "  the two single-term calls through engine      'cphase' (libbhnerf_eht.so) %.3f ms + 'logcamp' %.3f ms = %.3f ms"
                  % (cp_ms, lq_ms, cp_ms + lq_ms),
                  '  loss terms {total, amp, cphase, logcamp} = %s' % ', '.join('%.6e' % v for v in four)]
        if ns == 8:
            kept = dict(uv=uv, pairs=pairs)

    if not args.no_step:
        G4, FOV_M, B = 100, 16.0, NT
        geo = synthetic.synthetic_geodesics(NPIX, NPIX, G4, fov_M=FOV_M, inc_deg=60.0, seed=0)
        rt = network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                          t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr)
        pred = network.NeRF_Predictor(FOV_M / 2, 2.0, FOV_M / 2, 4.0, net_depth=4, net_width=256, mode='bf16', device=dev)
        t_frames = np.linspace(0.0, 1.0, B) * units.hr
        op = observation.ClosureDFT(kept['uv'], FOV, NPIX, pairs=kept['pairs'], triangles=observation.closure_triangles(8),
                                    quadrangles=observation.closure_quadrangles(8))
        cp = rng.uniform(-3, 3, (B, op.ncp)).astype(np.float32)
        lca = rng.normal(size=(B, op.nca)).astype(np.float32)
        data = {'cphase': (cp, np.full_like(cp, 0.1)), 'logcamp': (lca, np.full_like(lca, 0.1))}
        mk = lambda d: optimization.TrainStep.eht_closure(t_frames, kept['uv'], FOV, NPIX, kept['pairs'], d)
        combined = mk(data)
        added = mk({'cphase': data['cphase']}) + mk({'logcamp': data['logcamp']})
        assert combined.num_losses == 1 and added.num_losses == 2
        res = {}
        for name, step in (('combined', combined), ('added', added)):
            opt = optimization.Optimizer({'num_iters': 100, 'lr_init': 1e-4, 'lr_final': 1e-6}, pred, rt)
            res[name] = wall_ms(lambda: step(opt.state, rt, np.arange(B)))
            res[name + '_steps'] = int(opt.state.step)
        lines += ['training step, %d x %d rays x %d samples, 4x256 bf16, %d frames per step, 8 stations, wall time, median of 5 after 2 warm-ups:' % (NPIX, NPIX, G4, B),
                  "  ONE combined step   TrainStep.eht_closure('cphase+logcamp')                 %.2f ms  (%d Adam steps in 7 calls)"
                  % (res['combined'], res['combined_steps']),
                  "  TrainStep.__add__   eht_closure('cphase') + eht_closure('logcamp')          %.2f ms  (%d Adam steps in 7 calls)"
                  % (res['added'], res['added_steps']),
                  '  ratio added / combined %.2f' % (res['added'] / res['combined'])]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
