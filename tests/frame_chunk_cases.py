"""The problems of the frame-chunk tests (test_gpu_frame_chunks, and the bf16 cases of
test_gpu_backward.test_frame_group_taped_step_equals_full_step): the case tables, the ray sets and the builder.  No test here."""
import numpy as np
import torch

from conftest import mask_tie_points
from mlp_problems import f32r, stokes_factors, tilted_ray_grid
from oracle import oracle_np as onp

DENSE, SHELL = (8.0, 0.0, np.inf, np.inf), (8.0, 2.5, 8.0, 4.0)            # scale, rmin, rmax, z_width
RAY_SETS = {'dense 144': (12, 12, 32, DENSE), 'dense 96': (12, 8, 32, DENSE), 'compacted': (18, 15, 50, SHELL)}   # rays H x W, samples
T_FRAMES = (0.004, 0.021, 0.047)          # hours: t_M = t / GM_c3 + s + 5.6, so frame 0 is pre-injection for s < -6.3, frame 1 for s < -9.3
T_INJ = -(1000.0 - 4.0)

# name: (depth, width, mode, S, ray set, frames B, frames per pass)
CASES = {
    '4x128 S0 dense 144':        (4, 128, 'bf16', 0, 'dense 144', 3, (1, 2)),       # fused128; 2: uneven, passes of 2 + 1
    '4x128 S3 compacted':        (4, 128, 'bf16', 3, 'compacted', 3, (2,)),
    '4x100 S2 dense 96':         (4, 100, 'bf16', 2, 'dense 96', 2, (1,)),          # fused128, zero-padded
    '4x256 S0 dense 144':        (4, 256, 'bf16', 0, 'dense 144', 3, (1, 2)),       # ga0_chain, chain_slab_stage1
    '4x256 S3 dense 96':         (4, 256, 'bf16', 3, 'dense 96', 2, (1,)),          # ga0_chain, <= 16 chain workgroups
    '6x256 S1 compacted':        (6, 256, 'bf16', 1, 'compacted', 3, (2,)),         # ga0_chain, skip into layer 3
    '2x256 S0 dense 96':         (2, 256, 'bf16', 0, 'dense 96', 2, (1,)),          # generic, no W_out fold
    '6x64 S2 dense 144':         (6, 64, 'bf16', 2, 'dense 144', 3, (2,)),          # fold, resident chain
    '6x128 S0 dense 96':         (6, 128, 'bf16', 0, 'dense 96', 3, (1,)),          # fold, not fused128
    '4x256 f32 S3 dense 144':    (4, 256, 'f32', 3, 'dense 144', 3, (2,)),
    '4x64 f32 S0 dense 96':      (4, 64, 'f32', 0, 'dense 96', 3, (1,)),
    '8x32 f32 S0 dense 96':      (8, 32, 'f32', 0, 'dense 96', 3, (1,)),
    '4x256 f32 S4 dense 96':     (4, 256, 'f32', 4, 'dense 96', 3, (2,)),           # four planes: pass 2 reads dimages at 2 * 4 * R
}
# the problems of test_gpu_backward.test_frame_group_taped_step_equals_full_step's bf16 cases (three frames, groups of 2 + 1)
STEP_CASES = {'4x128 S0 dense 96': (4, 128, 'bf16', 0, 'dense 96', 3, ()), '4x256 S0 dense 96': (4, 256, 'bf16', 0, 'dense 96', 3, ())}

_PROBLEMS = {}


def problem(name):
    """The problem of a case in the layout of a g5_* fixture (float64 arrays of f32-rounded values; mlp_problems.tilted_ray_grid, as
    mlp_problems.random_problem) + the upstream image gradient `dimg` (B, Sx, R), rand - 0.4."""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    depth, width, mode, S, rays, B, _ = CASES[name] if name in CASES else STEP_CASES[name]
    H, Wd, G, dom = RAY_SETS[rays]
    _PROBLEMS[name] = build_problem(depth, width, mode, S, 3, H, Wd, G, dom, B)
    return _PROBLEMS[name]


def build_problem(depth, width, mode, S, deg, H, Wd, G, dom, B, do_skip=True, reseed=0, jitter=(0.0, 0.0, 0.0)):
    """The builder behind problem(): a network (depth x width, posenc degree `deg`; `mode` does not enter the problem) on H x Wd rays
    x G samples in the domain `dom`, B frames.  tests/buffer_contract_cases.py and tests/general_path_cases.py build their ray sets
    with it; the draws and their order are those of the frame-chunk cases (pinned by tests/test_buffer_contract_cases_cpu.py).
    do_skip False: the network without skip connections (general_path_cases); reseed: another draw of the same case; jitter:
    tilted_ray_grid's offsets, for the grids that otherwise put a sample on a mask boundary; B = 1: one frame, pre-injection samples in it."""
    rng = np.random.default_rng(1000 + 7 * width + depth + 31 * S + 100003 * reseed)
    geo, r = tilted_ray_grid(H, Wd, G, jitter)
    g = {k: f32r(v) for k, v in dict(geo, g=rng.uniform(0.6, 1.4, r.shape)).items()}
    g['J'] = f32r(stokes_factors(rng, r.shape, S)) if S else np.array(1.0)
    tree = onp.he_uniform_params(rng, depth, width, 3 + 6 * deg, do_skip=do_skip, dtype=np.float32)
    for i in range(depth + 1):
        g['kernel%d' % i] = tree['MLP_0']['Dense_%d' % i]['kernel'].astype(np.float64)
        g['bias%d' % i] = f32r(rng.uniform(-0.1, 0.1, tree['MLP_0']['Dense_%d' % i]['bias'].shape))
    g['bias%d' % depth] = g['bias%d' % depth] + 9.0              # (sigmoid(out - 10) off its flat tail)
    g.update(t_frames=np.array(T_FRAMES[:B]), t_start_obs=0.0, t_injection=T_INJ, hparams=np.array(list(dom) + [deg, depth, width, 1.0]))
    # no domain or injection mask decided within f32 rounding; pre-injection samples in frame 0, fewer of them in the last frame
    assert not mask_tie_points(g).any()
    tM = g['t_frames'].reshape(-1, 1, 1, 1) / onp.GM_C3_SGRA_HR + g['t_geos'] - T_INJ
    pre = (tM < 0).sum(axis=(1, 2, 3))
    assert len(set(T_FRAMES[:B])) == B and 0 < pre[0] < tM[0].size and (B == 1 or pre[-1] < pre[0])
    gen = torch.Generator().manual_seed(width + depth + S)
    dimg = (torch.rand((B, max(S, 1), H * Wd), generator=gen, dtype=torch.float64) - 0.4).float().double()
    return dict(g=g, dimg=dimg, dom=dom, depth=depth, width=width, S=S, B=B, spatial=(H, Wd))
