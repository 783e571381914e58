"""A/B of the backward's kernels (delta chain, dW, reduce) per library build at config 2's shape (128x128 rays x 64 samples, 8 frames),
from the events of bhn_render_bwd_tape_timed (bench.StepTimer: what bench.py's step timer reads), for several networks:

   python tools/ab_dw.py REF.so NEW.so [out.txt]     REF REF REF REF, then REF NEW REF NEW: every run a child process of
                                                     its own (BHNERF_HIP_LIB) under its own time limit; stops at the first that fails
   BHNERF_HIP_LIB=<lib> python tools/ab_dw.py child  one run: a JSON line {network: {kernel: median ms of STEPS calls}}

The first four runs give the box's run-to-run spread of a kernel (largest - smallest median of the same build); the verdict per
network and kernel is whether NEW's median (of its runs' medians) exceeds REF's (of its interleaved runs') by more than that."""
import json, os, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# depth, width, mode: the bf16 dW kernel of every width (6x128: 4x128 takes the fused backward), the 8-bit tape's, and the one form of
# the layer depth-1 job whose width-128 instance keeps three registers in scratch outside its group loop (3x128)
NETWORKS = [(4, 256, 'bf16'), (6, 128, 'bf16'), (6, 64, 'bf16'), (6, 32, 'bf16'), (4, 256, 'bf16_t8'), (3, 128, 'bf16')]
WARMUP, STEPS, CHILD_SECONDS = 5, 30, 240


def child():
    import torch
    from bench import StepTimer
    from bhnerf_amd import constants, engine, network, synthetic
    dev = torch.device('cuda:0')
    geo = synthetic.synthetic_geodesics(128, 128, 64, fov_M=16.0, inc_deg=60.0, seed=0)
    out = {}
    for depth, width, mode in NETWORKS:
        pred = network.NeRF_Predictor(8.0, 0.0, np.inf, np.inf, net_depth=depth, net_width=width, mode=mode, device=dev)
        eng = pred.engine()
        geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], None, geo['g'], geo['dtau'], geo['Sigma'])
        eng.pack(eng.flatten(network.MLP(depth, width).init(1, 21)))
        tM0 = engine.frame_offsets(np.linspace(0.0, 1.0, 64)[:8], 0.0, geo['t_injection'], constants.GM_c3('hr'), dev)
        dimg = torch.rand((8, 1, geom.R), generator=torch.Generator().manual_seed(3)).to(dev) * 1e-3
        assert eng.fits_tape(8, geom.P_eff)
        timer = StepTimer(eng)
        eng.step_timer = timer
        for rep in range(-WARMUP, STEPS):
            if rep == 0:
                torch.cuda.synchronize(); timer.reset()
            eng.render_train(geom, tM0)
            grad = eng.render_bwd_tape(geom, tM0, dimg)
        torch.cuda.synchronize()
        eng.step_timer = None
        assert torch.isfinite(grad).all()
        out['%dx%d %s' % (depth, width, mode)] = {n: round(float(np.median([e.elapsed(i, i + 1) for e in timer.bwd])), 4)
                                                  for i, n in enumerate(timer.names) if n != '-'}
        del eng, pred, geom
    print('AB_DW ' + json.dumps(out))


def run(lib):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], env=dict(os.environ, BHNERF_HIP_LIB=os.path.abspath(lib)),
                         capture_output=True, text=True, timeout=CHILD_SECONDS)
    lines = [l for l in res.stdout.splitlines() if l.startswith('AB_DW ')]
    if res.returncode != 0 or not lines:
        sys.exit('run with %s failed (exit %d):\n%s\n%s' % (lib, res.returncode, res.stdout[-2000:], res.stderr[-4000:]))
    return json.loads(lines[0][6:])


def main(ref, new, path=None):
    rows = []
    say = lambda s: (print(s, flush=True), rows.append(s))
    say('dW / reduce / chain kernel times per library build, config 2 (128x128 rays x 64 samples, 8 frames): median ms of %d calls per run,' % STEPS)
    say('bhn_render_bwd_tape_timed events; every run a process of its own.  ref = %s, new = %s' % (os.path.basename(ref), os.path.basename(new)))
    spread_runs = [run(ref) for _ in range(4)]
    ab = [(tag, run(lib)) for _ in range(2) for tag, lib in (('ref', ref), ('new', new))]
    worse = 0
    for net in spread_runs[0]:
        say('')
        say(net)
        for k in spread_runs[0][net]:
            s = [r[net][k] for r in spread_runs]
            a = [r[net][k] for t, r in ab if t == 'ref']
            b = [r[net][k] for t, r in ab if t == 'new']
            spread, ma, mb = max(s) - min(s), float(np.median(a)), float(np.median(b))
            verdict = 'within the spread' if mb - ma <= spread else 'SLOWER than ref + spread'
            worse += mb - ma > spread
            say('  %-44s ref x4 %s  spread %.4f | ref %s median %.4f | new %s median %.4f | new - ref %+.4f ms (%+.2f %%): %s' % (
                k[:44], ' '.join('%.4f' % v for v in s), spread, ' '.join('%.4f' % v for v in a), ma, ' '.join('%.4f' % v for v in b), mb,
                mb - ma, 100 * (mb - ma) / ma, verdict))
    say('')
    say('kernels slower than ref by more than the spread: %d' % worse)
    if path:
        open(path, 'w').write('\n'.join(rows) + '\n')
    return 1 if worse else 0


if __name__ == '__main__':
    if sys.argv[1] == 'child':
        child()
    else:
        sys.exit(main(*sys.argv[1:4]))
