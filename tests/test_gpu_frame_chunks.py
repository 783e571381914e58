"""GPU tests of the frame-chunked backward (`bhn_render_bwd` with a workspace that cannot hold the tape of all frames): the route
of every `RenderFunction.backward`.  Pass n > 0 runs with `BwdArgs::accumulate = 1` (csrc/fused_bwd.hip bwd_launch / bwd_pass): the
host offsets tM0 and dimages, clamps the later grids to the first pass's, calibrates the 8-bit tape on pass 0 only and reduces the
slabs once at the end; every kernel flush reads its slab back and adds.  A share that is stored instead of added changes ONE tensor,
far below the bf16 mode's bounds against the float64 oracle -- so each case here holds the CHUNKED gradient

* to its reference (mlp_reference.linear_reference's gradient): f32 against the float64 oracle inside mlp_bounds' GTOL / L2TOL
  (2e-5), bf16 against the emulator of the path that ran (gpu_support.assert_path) inside 4x the figures observed on the MI355X
  (OBSERVED; the kernels are bitwise reproducible), capped at mlp_bounds' CAPS['random'] (3e-3 whole gradient, 6e-3 worst tensor);
  ReLU ties adjudicated by mlp_bounds.held_or_adjudicated;
* to the all-at-once call on another predictor, per parameter tensor, rtol 1e-5 / atol 1e-6 of the tensor's largest entry
  (test_workspace_frame_chunking_is_equivalent's bound: the recomputed tape is the same point by point, only the order of the f32
  sums differs);
* to itself, repeated: bitwise equal.

Ray sets (the smallest that reach the branches): dense 12 x 12 rays x 32 samples = 144 groups per frame (18 tiles of eight: more
than 16 delta-chain workgroups in a one-frame pass, so chain_slab_stage1 runs; a multiple of 24, so the 8- and 12-group tilings and
with them the size query and the launch agree), dense 12 x 8 x 32 = 96 groups (12 tiles: the reduce without chain_slab_stage1), and
a point-compacted shell domain with 50 samples per ray (rays straddle groups).  Frame times are distinct with pre-injection samples
in the first frames, dimages differs in every frame and Stokes plane: a wrong frame or plane offset changes the result.
"""
import numpy as np
import pytest

from frame_chunk_cases import CASES, RAY_SETS, problem
from gpu_support import assert_path, dev, device_setup  # noqa: F401
from mlp_bounds import CAPS, GTOL, L2TOL, capped_bounds, expected_recipe, held_or_adjudicated, kernel_width, l2err, tensor_l2, tensor_label
from mlp_problems import tensor_cuts
from mlp_reference import dropped, linear_reference

pytestmark = pytest.mark.gpu

PARAMS = [(name, k) for name, c in CASES.items() for k in c[6]]
T8_BASE = '4x256 S0 dense 144'             # the 8-bit tape case: this problem in mode bf16_t8, one frame per pass

# Observed on the MI355X against the emulator, per bf16 case and frames per pass -- '<case name> k<frames per pass>': (relative L2 of
# the whole chunked gradient, worst relative L2 of one kernel / bias tensor; K0 in every case), as every case prints them.  The bound
# of a case is 4x its own figure, capped at CAPS['random'].
OBSERVED = {
    '4x128 S0 dense 144 k1': (9.87e-05, 3.69e-04),
    '4x128 S0 dense 144 k2': (9.87e-05, 3.69e-04),
    '4x128 S3 compacted k2': (1.31e-04, 3.64e-04),
    '4x100 S2 dense 96 k1':  (3.35e-05, 6.42e-05),
    '4x256 S0 dense 144 k1': (3.67e-05, 1.36e-04),
    '4x256 S0 dense 144 k2': (3.67e-05, 1.36e-04),
    '4x256 S3 dense 96 k1':  (2.04e-04, 5.30e-04),
    '6x256 S1 compacted k2': (2.57e-04, 5.10e-04),
    '2x256 S0 dense 96 k1':  (6.31e-06, 1.73e-05),
    '6x64 S2 dense 144 k2':  (8.96e-05, 3.32e-04),
    '6x128 S0 dense 96 k1':  (1.86e-04, 6.86e-04),
}


def bf16_bounds(key):
    b = capped_bounds(('grad', 'tensor'), OBSERVED[key], CAPS['random'])
    return b['grad'], b['tensor']


_RUNS = {}


def device_gradients(dev, name, prob, mode, recipe, compact, k, calls):
    """`calls` x eng.render_bwd on a FRESH predictor, on the fused path `recipe` (gpu_support.assert_path) -- all frames at once (k
    None), or with max_workspace_bytes = the size query for k frames -> (gradients, groups per frame)."""
    g, B = prob['g'], prob['B']
    pred, eng, geom, flat, tM0 = device_setup(g, mode, dev)
    P, gpf = geom.P_eff, geom.P_eff // 32
    assert_path(name, eng, geom, mode, recipe, False, compact=compact)
    if k is None:
        assert eng.fits_tape(B, P)
    else:
        q = eng._ws_bytes
        eng.max_workspace_bytes = q(k, P)
        assert not eng.fits_tape(B, P) and eng.tape_group(B, P) == k and eng.workspace(B, P).numel() == q(k, P)
        if geom.compact is not None:
            # the query sizes for the 8- AND the 12-group tiling, the launch for the one it runs: the query may exceed the launch's
            # need by the tape of at most 11 groups per frame.  One more frame costs more than k + 1 such margins, so the tape of
            # k + 1 frames does not fit the query for k in either tiling: THIS is what makes the launch stop at k frames per pass
            assert q(k + 1, P) - q(k, P) > (k + 1) * (q(1, P + 12 * 32) - q(1, P))
    eng.pack(flat)
    dimg = prob['dimg'].float().to(dev).contiguous()
    assert tuple(dimg.shape) == (B, geom.Sx, geom.R)
    grads = [eng.render_bwd(geom, tM0, dimg).cpu().numpy().astype(np.float64) for _ in range(calls)]
    return grads, gpf


def evaluate(dev, name, k, drop=None):
    """One case at k frames per pass: the problem, its reference (once), eng.render_bwd all at once and chunked on fresh predictors."""
    key = (name, k, drop is not None)
    if key in _RUNS:
        return _RUNS[key]
    depth, width, mode, S, rays, B, _ = CASES[name]
    prob = dropped(problem(name), drop)
    fkey = (name, None, drop is not None)
    recipe = expected_recipe(depth, kernel_width(width), False) if mode == 'bf16' else None
    run = lambda frames, calls: device_gradients(dev, name, prob, mode, recipe, rays == 'compacted', frames, calls)
    if fkey not in _RUNS:
        _RUNS[fkey] = run(None, 1)
    (full,), _ = _RUNS[fkey]
    (chunked, again), gpf = run(k, 2)
    assert gpf >= 96
    if rays == 'compacted':
        assert gpf >= 100 and RAY_SETS[rays][2] % 32 != 0
    else:
        assert gpf == int(rays.split()[1])
    gref = linear_reference('frame chunks', name, problem(name), recipe, drop)['grad']
    cuts = tensor_cuts(prob['g'], depth)
    spans = [(c0, c1) for c0, c1 in zip(cuts[:-1], cuts[1:])]
    assert cuts[-1] == gref.size == chunked.size and np.abs(gref).max() > 0
    tens = tensor_l2(chunked, gref, cuts, False)
    # against the all-at-once call, per tensor: the largest |difference| / (1e-6 max|full tensor| + 1e-5 |full|); must be <= 1
    vs_full = []
    for c0, c1 in spans:
        a, b = chunked[c0:c1], full[c0:c1]
        m = np.abs(b).max()
        vs_full.append(float((np.abs(a - b) / (1e-6 * m + 1e-5 * np.abs(b))).max()) if m > 0 else (0.0 if not a.any() else np.inf))
    passes = [k] * (B // k) + ([B % k] if B % k else [])
    r = dict(grad=l2err(chunked, gref), tensor=max(tens), gmax=float(np.abs(chunked - gref).max() / np.abs(gref).max()), vs_full=max(vs_full),
             repro=bool(np.array_equal(chunked, again)), chunked=chunked, recipe=recipe or 'f32', passes=passes)
    print('\n[frame chunks] %-24s %-9s %3d groups/frame  passes %-9s vs %s: L2 %.2e  max %.2e  worst tensor %.2e (%s)   vs all-at-once %.2f of '
          'the bound (%s)  repeat bitwise %s%s'
          % (name, r['recipe'], gpf, '+'.join(map(str, passes)), 'f64 oracle' if recipe is None else 'emulator', r['grad'], r['gmax'],
             r['tensor'], tensor_label(int(np.argmax(tens))), r['vs_full'], tensor_label(int(np.argmax(vs_full))), r['repro'],
             '' if drop is None else '  [tied samples taken out]'))
    _RUNS[key] = r
    return r


@pytest.mark.parametrize('name,k', PARAMS)
def test_chunked_backward_against_reference_and_all_at_once(dev, name, k):
    mode = CASES[name][2]
    if mode == 'f32':
        ok = lambda r: r['gmax'] < GTOL['f32'] and r['grad'] < L2TOL['f32']
    else:
        bg, bt = bf16_bounds('%s k%d' % (name, k))
        ok = lambda r: r['grad'] < bg and r['tensor'] < bt
    r = evaluate(dev, name, k)
    ref_ok, _ = held_or_adjudicated('%s, %d per pass' % (name, k), r, ok,
                                    lambda: linear_reference('frame chunks', name, problem(name), None if mode == 'f32' else r['recipe'], want_ties=True),
                                    lambda ties: evaluate(dev, name, k, drop=ties), lambda r2: r2['repro'] and r2['vs_full'] <= 1.0)
    # both comparisons are evaluated, and a failure reports both: which of them sees a fault is part of the finding
    figures = 'vs reference: L2 %.2e max %.2e worst tensor %.2e (%s); vs all-at-once: %.3g of the bound; repeat bitwise: %s' % (
        r['grad'], r['gmax'], r['tensor'], 'inside the bounds' if ref_ok else 'OUTSIDE the bounds', r['vs_full'], r['repro'])
    assert ref_ok and r['vs_full'] <= 1.0 and r['repro'], (name, k, figures)


def test_tape8_chunked_backward_calibrating_and_second_call(dev):
    """The 8-bit tape (bf16_t8) on the 4x256 dense 144 problem, one frame per pass: the first call on the workspace calibrates (on pass
    0 only: its scales come from frame 0 and serve frames 1 and 2), the second takes its scales from the first.  Both: finite, inside
    the bf16 mode's bounds against the float64 oracle, and within test_tape8_mode_gradient's 4e-2 of the bf16 mode's chunked
    gradient.  (Not compared with the all-at-once call, whose calibration sees other frames; the two calls differ in their scales.)"""
    prob = problem(T8_BASE)
    # the 8-bit tape folds W_out as the bf16 mode does but keeps dW_0 in dw_kernel (fused_bwd.hip ga0_chain_ok: its chain has no
    # registers to spare for the consumer), so this is the one case that runs dw_kernel's 8-bit flushes with accumulate = 1: path 't8'
    grads, gpf = device_gradients(dev, T8_BASE, prob, 'bf16_t8', 't8', False, 1, 2)
    assert gpf == 144
    gref = linear_reference('frame chunks', T8_BASE, prob, None)['grad']
    g16 = evaluate(dev, T8_BASE, 1)['chunked']
    for i, g8 in enumerate(grads):
        assert np.isfinite(g8).all()
        gmax, l2, d16 = float(np.abs(g8 - gref).max() / np.abs(gref).max()), l2err(g8, gref), l2err(g8, g16)
        print('\n[frame chunks] 4x256 bf16_t8 S0 dense 144  passes 1+1+1  call %d (%s): vs f64 oracle L2 %.2e  max %.2e   vs bf16 chunked %.2e'
              % (i, 'calibrating' if i == 0 else 'scales of call 0', l2, gmax, d16))
        assert gmax < GTOL['bf16'] and l2 < L2TOL['bf16'], (i, gmax, l2)
        assert d16 < 4e-2, (i, d16)
