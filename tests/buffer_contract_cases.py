"""The problems of the buffer-contract tests (test_gpu_buffer_contract; checked on the CPU by test_buffer_contract_cases_cpu): the ray
sets that reach the tails of the fused and general kernels, the case table (one case per backward path) and the builder.  No test here.

Ray sets, the smallest that reach the tails (50 samples per ray: rays straddle the 32-point groups):
  tiny       3 rays         150 points   5 groups: less than one 8-group tile, last group 22 points -- nearly every workgroup of
                                         every kernel is idle
  ragged     37 rays       1850 points   58 groups: 58 mod 8 = 2, 58 mod 12 = 10, last group 26 points
  compacted  frame_chunk_cases' SHELL set (18 x 15 rays): point-compacted; 3296 in-domain points = 103 whole groups (mod 8 = mod 12
             = 7), so this set has NO dom = 0 padding points
  compacted pad  the same domain on 17 x 15 rays: 3102 in-domain points = 97 groups (mod 8 = mod 12 = 1), the last one 30 points + 2
             dom = 0 padding points
  x12        1967 rays    98350 points   3074 groups (mod 12 = 2): the smallest dense set of 50-sample rays with a group count that is no
                                         multiple of 12 on which the fused 4x128 training forward runs 12-group tiles (it does from 3072
                                         groups per frame on; 1966 rays are 3072 groups, a multiple of 12)
Frames: three (frame_chunk_cases.T_FRAMES / T_INJ), pre-injection samples in frame 0, dimages different in every frame and plane."""
import numpy as np

from frame_chunk_cases import DENSE, SHELL, RAY_SETS as FC_RAY_SETS, build_problem
from mlp_reference import linear_reference

B = 3
# name: (rays H, rays W, samples, domain)
RAY_SETS = {'tiny': (3, 1, 50, DENSE), 'ragged': (37, 1, 50, DENSE), 'compacted': FC_RAY_SETS['compacted'], 'compacted pad': (17, 15, 50, SHELL),
            'x12': (7, 281, 50, DENSE)}
assert FC_RAY_SETS['compacted'][3] == SHELL
# what the ray sets must be (dense sets: points, 32-point groups, groups mod 8, groups mod 12, points in the last group)
RAGGED = {'tiny': (150, 5, 5, 5, 22), 'ragged': (1850, 58, 2, 10, 26), 'x12': (98350, 3074, 2, 2, 14),
          'compacted': (3296, 103, 7, 7, 32), 'compacted pad': (3102, 97, 1, 1, 30)}        # (compacted: the in-domain points)

# name: (depth, width, mode, S, posenc degree, ray set, recipe = the backward path, 32-point groups per tile of the training forward)
CASES = {
    '4x128 S0 tiny':            (4, 128, 'bf16', 0, 3, 'tiny', 'fused128', 8),
    '4x128 S3 x12':             (4, 128, 'bf16', 3, 3, 'x12', 'fused128', 12),
    '4x128 S0 deg0 ragged':     (4, 128, 'bf16', 0, 0, 'ragged', 'fused128', 8),       # unused encoding slots
    '4x100 S2 ragged':          (4, 100, 'bf16', 2, 3, 'ragged', 'fused128', 8),       # zero-padded
    '4x128 S0 compacted pad':   (4, 128, 'bf16', 0, 3, 'compacted pad', 'fused128', 8),   # the padding points of a compacted layout
    '4x256 S3 ragged':          (4, 256, 'bf16', 3, 3, 'ragged', 'ga0_chain', 8),
    '4x256 S0 tiny':            (4, 256, 'bf16', 0, 3, 'tiny', 'ga0_chain', 8),
    '6x256 S1 compacted':       (6, 256, 'bf16', 1, 3, 'compacted', 'ga0_chain', 8),   # skip into layer 3
    '6x64 S2 ragged':           (6, 64, 'bf16', 2, 3, 'ragged', 'fold', 8),            # resident chain
    '2x256 S0 ragged':          (2, 256, 'bf16', 0, 3, 'ragged', 'generic', 8),        # no W_out fold
    '4x64 f32 S0 tiny':         (4, 64, 'f32', 0, 3, 'tiny', 'f32', 4),
    '5x48 f32 S3 ragged':       (5, 48, 'f32', 3, 3, 'ragged', 'f32', 4),              # zero-padded to 64; odd depth: skip into the output layer
    '4x256 f32 S1 compacted':   (4, 256, 'f32', 1, 3, 'compacted', 'f32', 4),
    '4x256 t8 S0 ragged':       (4, 256, 'bf16_t8', 0, 3, 'ragged', 't8', 8),          # 8-bit tape
    '4x320 f32 S2 deg6 ragged': (4, 320, 'f32', 2, 6, 'ragged', 'general f32', 1),
    '4x320 S2 deg6 ragged':     (4, 320, 'bf16', 2, 6, 'ragged', 'general', 1),
    '5x40 f32 S3 deg10 tiny':   (5, 40, 'f32', 3, 10, 'tiny', 'general f32', 1),       # zero-padded
}

_PROBLEMS = {}


def problem(name):
    """frame_chunk_cases.build_problem's dict of a case (built once) + 'deg' and 'rays'."""
    if name not in _PROBLEMS:
        depth, width, mode, S, deg, rays, _, _ = CASES[name]
        H, Wd, G, dom = RAY_SETS[rays]
        _PROBLEMS[name] = dict(build_problem(depth, width, mode, S, deg, H, Wd, G, dom, B), deg=deg, rays=rays)
    return _PROBLEMS[name]


def domain_mask(prob):
    """(H, W, G) bool: the samples inside the recovery domain (emission.py:370-373 on the un-warped coordinates)."""
    c, (_, rmin, rmax, zw) = prob['g']['coords'], prob['dom']
    r2 = (c ** 2).sum(0)
    return ~((r2 < rmin ** 2) | (r2 > rmax ** 2) | (np.abs(c[2]) > zw))


def ragged_properties(name):
    """What the ray set of a case is, for the table's own checks: dense sets -> (points, groups, groups mod 8, groups mod 12, points in
    the last group); the compacted set -> the same of its in-domain points, as the engine lays them out (padded to whole groups)."""
    prob = problem(name)
    H, Wd, G, _ = RAY_SETS[prob['rays']]
    n = H * Wd * G if not prob['rays'].startswith('compacted') else int(domain_mask(prob).sum())
    groups = (n + 31) // 32
    return n, groups, groups % 8, groups % 12, n - 32 * (groups - 1)


def check_table():
    """The properties the case table promises; raises AssertionError."""
    for name, (depth, width, mode, S, deg, rays, recipe, nwf) in CASES.items():
        prob = problem(name)
        assert prob['B'] == B == 3 and prob['dimg'].shape == (B, max(S, 1), prob['spatial'][0] * prob['spatial'][1])
        d = prob['dimg'].numpy().reshape(B * max(S, 1), -1)
        assert all(not np.array_equal(d[i], d[j]) for i in range(len(d)) for j in range(i)), name     # every frame and plane differs
        props = ragged_properties(name)
        assert props == RAGGED[rays], (name, props)
        if rays.startswith('compacted'):
            H, Wd, G, _ = RAY_SETS[rays]
            # point-compacted by the engine (less than 0.9 of the samples in the domain), rays straddle groups; 'pad': dom = 0 padding points
            assert 0 < props[0] < 0.9 * H * Wd * G and G % 32 != 0 and (props[0] % 32 != 0) == (rays == 'compacted pad'), (name, props)
        else:
            assert RAY_SETS[rays][2] == 50 and props[4] != 32 and (rays == 'x12' or props[1] < 96)
    assert RAGGED['tiny'][1] < 8 and RAGGED['x12'][1] % 12 != 0 and RAGGED['x12'][1] >= 3072


# ---- references: mlp_reference.linear_reference, the float64 oracle (recipe None) or the bf16 emulator of the path that runs
def reference(name, recipe=None, drop=None, want_ties=False):
    return linear_reference('buffer contract', name, problem(name), recipe, drop, want_ties=want_ties)
