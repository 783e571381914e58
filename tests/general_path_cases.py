"""The problems of the general-path tests (test_gpu_general_path; checked on the CPU by test_general_path_cases_cpu): the case table --
one case per branch of csrc/general_mlp.hip's host rules that the older suite never holds to a reference --, its ray sets, the
builder, the references and a Python restatement of those host rules (gen_layout, gen_block, gen_lds16_bytes, gen_ng16, the strips of
gen_dw_kernel / gen_dw16_kernel, the chunks of gen_backward, fused_fwd.hip's ray_direct).  No test here.

Ray sets (tiny, ragged, compacted: buffer_contract_cases'; 50-sample rays straddle the 32-point groups):
  direct 64        7 x 5 rays x 64 samples, dense: every ray starts on a group boundary and is two groups long -- ray_direct
  direct 33        11 x 5 rays x 33 samples, dense: rays of at most 33 samples touch at most two groups anywhere -- ray_direct
  long 257         3 x 3 rays x 257 samples, dense: 2313 points = 73 groups; the longest ray that lies in at most two 8-group tiles
                   (DESIGN.md 4.7's bitwise claim), every ray runs through all eight groups of a tile
  compacted span2  12 x 12 rays x 32 samples in the shell domain: point-compacted, no ray has more than 32 in-domain points, so
                   bhn_geom.ray_span <= 2 -- ray_direct with a ray index
  compacted 100    8 x 6 rays x 100 samples in the shell domain: up to 63 in-domain points per ray, ray_span 3 as it comes out --
                   NOT direct (the shell set of the buffer-contract cases, `compacted`, has ray_span 2: direct as well)
The sample grids of 33, 64, 100 and 257 points put one sample per ray within f32 rounding of t_M = 0 in one frame; those sets are shifted by
JITTER along the ray (tilted_ray_grid's jitter).  Every set stays under 4,000 (in-domain) points per frame.  Frames: frame_chunk_cases.T_FRAMES (B = 3; one case has B = 1)."""
import numpy as np

import buffer_contract_cases as bc
from frame_chunk_cases import DENSE, SHELL, build_problem
from mlp_bounds import GTOL, L2TOL, caps_of
from mlp_reference import linear_reference

RAY_SETS = dict({k: bc.RAY_SETS[k] for k in ('tiny', 'ragged', 'compacted')},
                **{'direct 64': (7, 5, 64, DENSE), 'direct 33': (11, 5, 33, DENSE), 'long 257': (3, 3, 257, DENSE),
                   'compacted span2': (12, 12, 32, SHELL), 'compacted 100': (8, 6, 100, SHELL)})
JITTER = {'direct 64': (0.0, 0.0, 0.013), 'direct 33': (0.011, 0.007, 0.013), 'long 257': (0.011, 0.007, 0.013),
          'compacted 100': (0.0, 0.0, 0.013)}
# bhn_geom.ray_span of the compacted sets, as engine.ray_span gives it (restated by ray_span() below; recorded here, pinned by the CPU test)
RAY_SPAN = {'compacted': 2, 'compacted span2': 2, 'compacted 100': 3}

# name: (depth, width, posenc degree, S, ray set, frames B, do_skip, reseed)
CASES = {
    '4x32 deg5 S0 ragged':            (4, 32, 5, 0, 'ragged', 3, True, 0),         # MTp 1 on two waves; nt 1; F 33: 31 zero slots
    '3x96 deg6 S2 ragged':            (3, 96, 6, 2, 'ragged', 3, True, 0),         # MTp 3; nt 3; skip into layer 2 and the output layer
    '4x160 deg5 S3 compacted':        (4, 160, 5, 3, 'compacted', 3, True, 0),     # MTp 5 on four waves; strips 4 + 1
    '4x160 deg5 S0 noskip ragged':    (4, 160, 5, 0, 'ragged', 3, False, 0),       # erows only in layer 0
    '6x224 deg7 S1 ragged':           (6, 224, 7, 1, 'ragged', 3, True, 0),        # MTp 7; strips 4 + 3; depth 6
    '4x256 deg5 S2 ragged':           (4, 256, 5, 2, 'ragged', 3, True, 0),        # MTp 8: 512 threads with NG 4; five octaves over nsub 4
    '4x288 deg3 S2 ragged':           (4, 288, 3, 2, 'ragged', 3, True, 0),        # the largest NG 4 launch; MTp 9 on eight waves; Ep 32
    '4x257 deg5 S0 ragged':           (4, 257, 5, 0, 'ragged', 3, True, 0),        # Wp 288 at NG 2; 31 zero-padded columns
    # (2,400 hidden units see 150 ray samples in three frames: 0.26 ... 0.35 of the samples have a ReLU tie in most draws -- the 96th draw has 37)
    '5x480 deg0 S2 tiny':             (5, 480, 0, 2, 'tiny', 3, True, 95),         # MTp 15; nt 3; F 3: no octave; odd depth
    '2x33 deg10 S3 tiny B1':          (2, 33, 10, 3, 'tiny', 1, True, 0),          # Wp 64 with 31 padded columns; F 63; total_tiles 1
    '4x416 deg9 S1 compacted':        (4, 416, 9, 1, 'compacted', 3, True, 0),     # MTp 13; strips 4 + 4 + 4 + 1
    '4x128 deg5 S3 direct 64':        (4, 128, 5, 3, 'direct 64', 3, True, 0),     # ray_direct, dense G 64
    '4x320 deg6 S0 direct 64':        (4, 320, 6, 0, 'direct 64', 3, True, 0),     # the same at NG 2
    '4x128 deg5 S0 direct 33':        (4, 128, 5, 0, 'direct 33', 3, True, 0),     # ray_direct, G <= 33
    '4x320 deg6 S2 long 257':         (4, 320, 6, 2, 'long 257', 3, True, 0),      # the combine over all eight groups of a tile
    '4x128 deg5 S2 compacted span2':  (4, 128, 5, 2, 'compacted span2', 3, True, 0),   # ray_direct with ray_idx
    '4x128 deg5 S2 compacted 100':    (4, 128, 5, 2, 'compacted 100', 3, True, 0),     # ... and the other side of that rule: ray_span 3
}
MODES = ('f32', 'bf16')
CHUNK_SWEEP = ('3x96 deg6 S2 ragged', '4x257 deg5 S0 ragged', '4x416 deg9 S1 compacted')       # NG 4, NG 2, compacted
CHUNK_TILES = (2, 3, 5, -1)              # tiles of tape in the workspace; -1: the tile count minus one

_PROBLEMS = {}


def problem(name):
    """frame_chunk_cases.build_problem's dict of a case (built once) + 'deg', 'rays' and 'do_skip'."""
    if name not in _PROBLEMS:
        depth, width, deg, S, rays, B, do_skip, reseed = CASES[name]
        H, Wd, G, dom = RAY_SETS[rays]
        _PROBLEMS[name] = dict(build_problem(depth, width, 'f32', S, deg, H, Wd, G, dom, B, do_skip=do_skip, reseed=reseed,
                                             jitter=JITTER.get(rays, (0.0, 0.0, 0.0))),
                               deg=deg, rays=rays, do_skip=do_skip)
    return _PROBLEMS[name]


def reference(name, mode, drop=None, want_ties=False, accum32=False):
    """mlp_reference.linear_reference of a case: the float64 oracle for mode 'f32', the emulator of the `general` recipe for 'bf16'."""
    return linear_reference('general path', name, problem(name), None if mode == 'f32' else 'general', drop, accum32, want_ties)


def in_domain(name):
    """(H, W, G) bool: the ray samples inside the recovery domain."""
    return bc.domain_mask(problem(name))


def points_per_frame(name):
    """Points the kernels visit per frame: every sample of a dense set, the in-domain ones of a compacted set."""
    H, Wd, G, _ = RAY_SETS[CASES[name][4]]
    return int(in_domain(name).sum()) if CASES[name][4].startswith('compacted') else H * Wd * G


# ---- the host rules of csrc/general_mlp.hip, restated
def ray_span(mask):
    """engine.ray_span of a point-compacted layout from the (H, W, G) in-domain mask: the most consecutive 32-point groups the
    in-domain points of one ray lie in (0: no point)."""
    n = mask.reshape(-1, mask.shape[-1]).sum(axis=1)
    start = np.cumsum(n) - n
    n, start = n[n > 0], start[n > 0]
    return int(((start + n - 1) // 32 - start // 32).max()) + 1 if n.size else 0


def ray_direct(G, span=None):
    """fused_fwd.hip's rule: the render adds every group's ray segments straight to the pixels (no combine in LDS) -- span None:
    a dense layout of G samples per ray; else a compacted layout with that bhn_geom.ray_span."""
    return span in (1, 2) if span is not None else (G <= 33 or (G <= 64 and G % 32 == 0))


def skip_inputs(depth, do_skip):
    """skip_in[l] of bhn_mlp_shape (network.py:59-61): layer l takes concat[h_l, enc]."""
    s = [False] * (depth + 1)
    for i in range(1, depth):
        if do_skip and i % (depth // 2) == 0:
            s[i + 1] = True
    return s


def layout(depth, width, deg, do_skip, Sx):
    """gen_layout + gen_block + gen_lds16_bytes + gen_ng16 + the strips of the weight-gradient kernels, as a dict."""
    F = 3 + 6 * deg
    Wp, Ep = (width + 31) // 32 * 32, (F + 31) // 32 * 32
    MTp = Wp // 32
    block = 512 if MTp >= 8 else 256 if MTp >= 4 else 128
    raysum = 8 * 32 * 4 + 8 * Sx * 32 * 4 + 8 * 4                                     # RaySum<8>::bytes(Sx)
    lds16 = lambda ng: ng * (2 * Wp * 64 + Ep * 64) + ng * 32 * 4 * 3 + raysum
    NG = 4 if lds16(4) <= 160 * 1024 else 2
    skip = skip_inputs(depth, do_skip)
    layers, packed, slab, njobs, o16 = [], 0, 0, 0, 0
    for l in range(depth + 1):
        hrows, erows, outp = (Wp if l > 0 else 0), (Ep if l == 0 or skip[l] else 0), (32 if l == depth else Wp)
        nst = (outp // 32 + 3) // 4
        layers.append(dict(hrows=hrows, erows=erows, outp=outp, nt=[min(4, outp // 32 - 4 * s) for s in range(nst)],
                           h_true=width if l > 0 else 0, e_true=F if erows else 0))
        packed += (hrows + erows) * outp + (outp * hrows if 1 <= l < depth else 0) + outp
        slab += (hrows + erows + 32) * outp
        njobs += ((hrows + erows) // 32 + 1) * nst
        o16 += (outp // 32) * ((hrows + erows) // 16) * 1024 + ((hrows // 32) * (outp // 16) * 1024 if 1 <= l < depth else 0)
    nsplit = min(256, max(8, (6144 + njobs - 1) // njobs))
    tape_f32 = 4 * (Ep * 32 + 2 * depth * Wp * 32 + 1024 + 32)                      # bytes of one group's tape
    tape_bf16 = (Ep // 32) * 2048 + 2 * depth * MTp * 2048 + depth * MTp * 256 + 256
    image_off = (packed * 4 + 255) // 256 * 256
    return dict(F=F, Wp=Wp, Ep=Ep, MTp=MTp, block=block, waves=block // 64, NG=NG, lds16=lds16(NG), lds16_at_4=lds16(4), nsub=block // 32 // NG,
                lds_f32=(2 * Wp + Ep) * 32 * 4 + (16 * 32 + 64) * 4 + raysum, layers=layers, njobs=njobs, nsplit=nsplit,
                slab_bytes=(nsplit * slab * 4 + 255) // 256 * 256, tape_bytes={'f32': tape_f32, 'bf16': tape_bf16},
                packed_bytes={'f32': packed * 4, 'bf16': image_off + o16})


def case_layout(name):
    depth, width, deg, S, rays, B, do_skip, _ = CASES[name]
    L = layout(depth, width, deg, do_skip, max(S, 1))
    groups = (points_per_frame(name) + 31) // 32
    tiles = (groups + 7) // 8                                                        # tiles of eight groups per frame
    G = RAY_SETS[rays][2]
    span = ray_span(in_domain(name)) if rays.startswith('compacted') else None
    return dict(L, groups=groups, tiles_per_frame=tiles, total_tiles=tiles * B, ray_span=span, ray_direct=ray_direct(G, span))


def workspace_bytes(name, mode, tiles):
    """Slabs + `tiles` tiles of tape: what bhn_render_bwd_workspace_bytes reports for tiles = every tile of the call, and the least
    bhn_render_bwd accepts for tiles = min(total_tiles, 2)."""
    L = case_layout(name)
    return L['slab_bytes'] + tiles * 8 * L['tape_bytes'][mode]


def chunks(total_tiles, k):
    """gen_backward's passes for a workspace of slabs + k tiles of tape: [(first tile, tiles, accumulate)]."""
    return [(c0, min(k, total_tiles - c0), c0 > 0) for c0 in range(0, total_tiles, k)]


def cuts_a_frame(chunk, tiles_per_frame):
    """The pass holds tiles of more than one frame."""
    return chunk[0] // tiles_per_frame != (chunk[0] + chunk[1] - 1) // tiles_per_frame


# ---- bounds: none comes from the kernels under test
def bounds(name, mode):
    """f32 against the float64 oracle: gpu_support.check_general_path_problem's figures; bf16 against the emulator: mlp_bounds'
    caps of the 'random' class (the emission, which has no cap of its own, at the image cap: an image is a weighted sum of emissions)."""
    deg = CASES[name][2]
    k = max(1.0, 2.0 ** (deg - 5))
    if mode == 'f32':
        return dict(image=1e-5 * k, emission=1e-5 * k, gmax=GTOL['f32'] * k, grad=L2TOL['f32'] * k)
    cap = caps_of('random', deg)
    return dict(cap, emission=cap['image'])
