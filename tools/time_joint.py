#!/usr/bin/env python3
"""Time the joint training step (optimization.TrainStep.joint) against the sum of the same terms (TrainStep.__add__) on the device,
in one process, on the same state and ray set:

  config-4 shape     256 x 256 rays x 100 samples, Stokes I/Q/U, 4x256 bf16, 8 frames per step, 8 stations (28 baselines):
                     eht_closure('cphase+logcamp') on the I plane and eht_pol('m') -- the terms of `eht_recovery.py --stokes --gains`
  example defaults   32 x 32 rays x 64 samples, 4x128 bf16, 64 frames in batches of 6, the ngEHT table: eht_obs('vis') and
                     volume_prior({'tv': 1}) on a 32^3 lattice -- the terms of `eht_recovery.py --tv W`

`a + b` renders, runs a backward and takes an Adam step once per term; `TrainStep.joint(a, b)` renders each group once, adds the
gradients (bhn_jnt_sum) and takes one Adam step.  Per combination: warm-ups of both, then ROUNDS alternated rounds of ITERS
iterations each, a host clock around work that ends in a device synchronise; the median round of each and the spread (min .. max)
of its rounds are reported in ms per iteration.  Nothing is asserted on time.  Writes profiles/joint_step_time.txt (or --out).

  python tools/time_joint.py [--out profiles/joint_step_time.txt] [--small]

--small runs both combinations at toy sizes (a rehearsal of the script; its times are times of overheads).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
from bhnerf_amd import network, observation, optimization, synthetic, units        # noqa: E402
from time_eht_uv import FOV                                                       # noqa: E402

ROUNDS = 5
FOV_M = 16.0


def ray_set(size, samples, stokes):
    geo = synthetic.synthetic_geodesics(size, size, samples, fov_M=FOV_M, inc_deg=60.0, seed=0, **(dict(S=3) if stokes else {}))
    return network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                        t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr,
                                   **(dict(J=geo['J']) if stokes else {}))


def alternated(variants, state, rt, batch, iters, warmup):
    """{name: [ms per iteration of each round]}: the variants take turns, round after round, on one state."""
    out = {name: [] for name in variants}
    for name, step in variants.items():
        for _ in range(warmup):
            _, state, _ = step(state, rt, step.args[0].sample(batch))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, step in variants.items():
            frames = step.args[0]
            t0 = time.perf_counter()
            for _ in range(iters):
                _, state, _ = step(state, rt, frames.sample(batch))
            torch.cuda.synchronize()
            out[name].append(1e3 * (time.perf_counter() - t0) / iters)
    return out


def report(title, res, iters):
    lines = [title, '  %d alternated rounds of %d iterations each; ms per iteration: median round (min .. max of the rounds)' % (ROUNDS, iters)]
    for name, ms in res.items():
        lines.append('  %-58s %8.3f  (%.3f .. %.3f)' % (name, float(np.median(ms)), min(ms), max(ms)))
    a, b = (float(np.median(ms)) for ms in res.values())
    spread = max(max(ms) - min(ms) for ms in res.values())
    lines.append('  joint - sum: %+.3f ms per iteration (%+.1f %%); the largest spread of a variant over its rounds: %.3f ms' % (b - a, 100.0 * (b - a) / a, spread))
    return lines


def gains_combination(dev, small):
    size, samples, width, B, stations = (16, 16, 128, 2, 5) if small else (256, 100, 256, 8, 8)
    rng = np.random.default_rng(0)
    rt = ray_set(size, samples, stokes=True)
    pred = network.NeRF_Predictor(FOV_M / 2, 2.0, FOV_M / 2, 4.0, net_depth=4, net_width=width, mode='bf16', device=dev)
    t_frames = np.linspace(0.0, 1.0, B) * units.hr
    pos = rng.normal(size=(B, stations, 2)) * 3e9
    pairs = np.array([(i, j) for i in range(stations) for j in range(i + 1, stations)])
    uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])
    tri, quad = observation.closure_triangles(stations), observation.closure_quadrangles(stations)
    data = {}
    for term, n in (('cphase', len(tri)), ('logcamp', len(quad))):
        sigma = np.full((B, 3, n), 0.2, dtype=np.float32)
        sigma[:, 1:] = np.inf                                 # the Q and U planes of the closure step carry no weight
        data[term] = (rng.uniform(-1.0, 1.0, (B, 3, n)).astype(np.float32), sigma)
    closure = optimization.TrainStep.eht_closure(t_frames, uv, FOV, size, pairs, data, triangles=tri, quadrangles=quad)
    m = (0.3 * (rng.normal(size=(B, len(pairs))) + 1j * rng.normal(size=(B, len(pairs))))).astype(np.complex64)
    pol = optimization.TrainStep.eht_pol(t_frames, uv, FOV, size, {'m': (m, np.full(m.shape, 0.1, dtype=np.float32))})
    opt = optimization.Optimizer({'num_iters': 100000, 'lr_init': 1e-4, 'lr_final': 1e-6}, pred, rt)
    iters = 3 if small else 20
    res = alternated({"eht_closure('cphase+logcamp') + eht_pol('m')": closure + pol,
                      "TrainStep.joint(eht_closure('cphase+logcamp'), eht_pol('m'))": optimization.TrainStep.joint(closure, pol)},
                     opt.state, rt, B, iters, warmup=3)
    return report("config-4 shape: %d x %d rays x %d samples, I/Q/U, 4x%d bf16, %d frames per step, %d stations (%d baselines, %d triangles, %d quadrangles)"
                  % (size, size, samples, width, B, stations, len(pairs), len(tri), len(quad)), res, iters)


def prior_combination(dev, small):
    size, samples, nt, B, res3 = (16, 16, 8, 2, 8) if small else (32, 64, 64, 6, 32)
    rng = np.random.default_rng(1)
    rt = ray_set(size, samples, stokes=False)
    pred = network.NeRF_Predictor(FOV_M / 2, 2.0, FOV_M / 2, 4.0, net_depth=4, net_width=128, mode='bf16', device=dev)
    tstart, tstop = 2.0, 2.0 + 40.0 / 60.0
    array = observation.Array.load_txt(os.path.join(ROOT, 'tests', 'golden', 'eht_arrays', 'ngEHT.txt'))
    obs = observation.empty_eht_obs(times=np.linspace(tstart, tstop, nt), mjd=57851, timetype='GMST', nt=nt, tstart=tstart, tstop=tstop, tint=30.0, array=array)
    vis = (0.05 * (rng.normal(size=(nt, obs.nvis)) + 1j * rng.normal(size=(nt, obs.nvis)))).astype(np.complex64)
    t_frames = np.linspace(tstart, tstop, nt) * units.hr
    data = optimization.TrainStep.eht_obs(t_frames, obs, vis, FOV, size, dtype='vis')
    prior = optimization.TrainStep.volume_prior(FOV_M, resolution=res3, weights={'tv': 1.0}, scale=1e3)
    opt = optimization.Optimizer({'num_iters': 100000, 'lr_init': 1e-4, 'lr_final': 1e-6}, pred, rt)
    iters = 5 if small else 400
    res = alternated({"eht_obs('vis') + volume_prior({'tv': 1})": data + prior,
                      "TrainStep.joint(eht_obs('vis'), volume_prior({'tv': 1}))": optimization.TrainStep.joint(data, prior)},
                     opt.state, rt, B, iters, warmup=20)
    return report("examples/eht_recovery.py defaults: %d x %d rays x %d samples, 4x128 bf16, %d frames in batches of %d, ngEHT (%d baselines), tv lattice %d^3"
                  % (size, size, samples, nt, B, obs.nvis, res3), res, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_step_time.txt'))
    ap.add_argument('--small', action='store_true', help='toy sizes: a rehearsal of the script')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    lines = ['joint step against the sum of the same terms, host clock around steps that end in a device synchronise (%s)%s'
             % (torch.cuda.get_device_name(0), ' -- TOY SIZES' if args.small else '')]
    lines += gains_combination(dev, args.small)
    lines += prior_combination(dev, args.small)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
