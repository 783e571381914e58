#!/usr/bin/env python3
"""Time the polarimetric EHT losses (libbhnerf_pol.so, observation.PolDFT) on the device, in one process:

  shape      8 frames x 3 Stokes planes x 256 x 256 pixels, an 8-station array: 28 baselines (24 planes per call)
  measured   'm' and 'pvis+m' with the image gradient: the library call alone (every buffer allocated once) and the same call
             through engine.chi2_eht; the forward-only library call beside them
  yardstick  bhn_eht_chi2_uv 'vis' with the gradient on the same 24 planes (Sx = 3: three complex visibility fits per frame,
             the twiddle tables, forward pass and adjoint of the same kernels), library call alone and through engine

3 warm-ups, median of 10 event-timed calls each.  Nothing is asserted on time.  Writes profiles/pol_time.txt (or --out).

  python tools/time_pol.py [--out profiles/pol_time.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
from bhnerf_amd import _hip, engine, observation        # noqa: E402
from time_eht_uv import FOV, NPIX, NT, array, median_ms  # noqa: E402

SX = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pol_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(NPIX) - 127.5, np.arange(NPIX) - 127.5, indexing='ij')
    img = np.exp(-0.5 * (yy ** 2 + xx ** 2) / 12.0 ** 2)[None, None] + 0.05 * rng.uniform(size=(NT, SX, NPIX, NPIX))
    img = img * (2.0 / img.sum(axis=(2, 3), keepdims=True)) * np.array([1.0, 0.3, -0.2])[None, :, None, None]
    images = torch.as_tensor(img.astype(np.float32), device=dev)
    uv, _ = array(8, rng)
    nvis, N = uv.shape[1], NT * SX
    pol = observation.PolDFT(uv, FOV, NPIX).to(dev)
    plain = observation.DirectDFT(uv, FOV, NPIX).to(dev)
    vis = pol.observe(images).cpu().numpy()
    lines = ["polarimetric EHT losses + image gradient per call, %d frames x %d Stokes planes x %d x %d pixels, %d baselines, median of 10 "
             'event-timed calls after 3 warm-ups (%s)' % (NT, SX, NPIX, NPIX, nvis, torch.cuda.get_device_name(0))]
    st, psize = _hip.stream_ptr(dev), FOV / NPIX

    # the polarimetric library: targets off the model by a few sigma
    held = {}
    for t, q in (('pvis', pol.polarised_visibility(vis)), ('m', pol.fractional_polarisation(vis))):
        tgt = torch.as_tensor((q * (1.0 + 0.1 * rng.normal(size=q.shape))).astype(np.complex64), device=dev)
        held[t] = (tgt, torch.full(q.shape, 0.05 * float(np.abs(q).mean()), dtype=torch.float32, device=dev))
    lib = _hip.pol_lib()
    nb = int(lib.bhn_pol_ws_bytes(N, nvis, NPIX, NPIX))
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    loss3, dimg = torch.empty((3,), dtype=torch.float32, device=dev), torch.empty_like(images)
    structs = {t: _hip.bhn_pol_term(v[0].data_ptr(), v[1].data_ptr(), 1.0) for t, v in held.items()}
    lines.append('libbhnerf_pol.so, workspace %.2f MB' % (nb / 1e6))
    for dtype in ('m', 'pvis+m'):
        terms = dtype.split('+')
        ref = lambda t: C.byref(structs[t]) if t in terms else None
        call = lambda grad=True: _hip.pol_check(lib.bhn_pol_chi2(
            _hip.ptr(images), _hip.ptr(pol.uv), N, SX, nvis, NPIX, NPIX, psize, psize, ref('pvis'), ref('m'), 1.0, _hip.ptr(loss3),
            _hip.ptr(dimg) if grad else None, _hip.ptr(ws), nb, st))
        tgt, sig = torch.cat([held[t][0] for t in terms], dim=-1), torch.cat([held[t][1] for t in terms], dim=-1)
        lib_ms, fwd_ms = median_ms(call), median_ms(lambda: call(False))
        eng_ms = median_ms(lambda: engine.chi2_eht(images, pol, tgt, sig, 1.0, dtype))
        three = pol.last_terms.cpu().numpy()
        lines += ["  '%s'" % dtype,
                  '    library call alone (buffers allocated once)   %.3f ms with the gradient, %.3f ms forward only' % (lib_ms, fwd_ms),
                  "    engine.chi2_eht(.., '%s')%s %.3f ms" % (dtype, ' ' * (20 - len(dtype)), eng_ms),
                  '    loss terms {total, pvis, m} = %s' % ', '.join('%.6e' % v for v in three)]

    # the yardstick: 'vis' on the same 24 planes through libbhnerf_eht.so
    vt = torch.as_tensor((vis * (1.0 + 0.1 * rng.normal(size=vis.shape))).astype(np.complex64), device=dev)
    vs = torch.full(vis.shape, 0.05 * float(np.abs(vis).mean()), dtype=torch.float32, device=dev)
    elib = _hip.eht_lib()
    enb = int(elib.bhn_eht_ws_bytes(N, nvis, 0, NPIX, NPIX))
    ews = torch.empty((enb,), dtype=torch.uint8, device=dev)
    loss1 = torch.empty((1,), dtype=torch.float32, device=dev)
    vcall = lambda grad=True: _hip.eht_check(elib.bhn_eht_chi2_uv(
        _hip.ptr(images), _hip.ptr(plain.uv), N, SX, nvis, NPIX, NPIX, psize, psize, engine.EHT_DTYPES['vis'], _hip.ptr(vt), _hip.ptr(vs), 1.0, None,
        None, 0, _hip.ptr(loss1), _hip.ptr(dimg) if grad else None, _hip.ptr(ews), enb, st))
    v_ms, vf_ms = median_ms(vcall), median_ms(lambda: vcall(False))
    ve_ms = median_ms(lambda: engine.chi2_eht(images, plain, vt, vs, 1.0, 'vis'))
    lines += ["yardstick: libbhnerf_eht.so 'vis' on the same %d planes, workspace %.2f MB" % (N, enb / 1e6),
              '    library call alone (buffers allocated once)   %.3f ms with the gradient, %.3f ms forward only' % (v_ms, vf_ms),
              "    engine.chi2_eht(.., 'vis')                    %.3f ms" % ve_ms,
              '    loss = %.6e' % loss1.item()]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
