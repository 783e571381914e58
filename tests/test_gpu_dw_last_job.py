"""GPU tests of the bf16 dW kernel's layer depth-1 job (fused_bwd.hip dw_body2 LAST: gA_{depth-1} rebuilt from h_depth and dout, the
output layer's row and bias riding on it) at width 256, where it runs on a wave grid of its own (8 x 1: one A tile and all eight B
tiles per wave) while every other job keeps 4 x 2.

With do_skip the form of the job follows from the depth, so depths 3 to 6 run its four instantiations:
    3  skip-concat into layer depth-1 and into the output layer      5  into the output layer only
    4  into layer depth-1                                            6  neither
Every case is mlp_problems.random_problem's ragged grid (9 x 7 rays x 50 samples, three frames, a point-compacted shell domain: 672
in-domain points = 21 groups per frame, 63 in all), so the layer depth-1 job's workgroups -- a fifth (depth 6) to a half (depth 3) of
one per CU, some 55 to 125 of 256 -- are about as many as the groups or more: a share holds two groups, one (the prologue, then one
body whose next group does not exist: `live_next`) or none (q0 == q1).  No tolerance is new: against the float64 oracle the bounds of test_random_problem_f32_and_bf16 (IMG_TOL / GTOL /
L2TOL['bf16']) on the chi^2 step, against the emulator of the path that ran (mlp_reference.point_reference) the caps of class
'random' (mlp_bounds.CAPS) on the recorded-tape route with an upstream gradient that differs in every frame and plane; ReLU ties
are adjudicated by mlp_bounds.held_or_adjudicated.  Every case runs twice on fresh predictors and is bitwise equal to itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_tree
from frame_chunk_cases import SHELL, build_problem
from gpu_support import assert_path, dev, device_setup, predictor_of, random_problem_errors, ray_args  # noqa: F401
from mlp_bounds import CAPS, GTOL, IMG_TOL, L2TOL, expected_recipe, first_difference, held_or_adjudicated, kernel_width, l2err, maxerr, tensor_l2
from mlp_problems import RANDOM_PROBLEM_DOMAIN, RANDOM_PROBLEM_SHAPE, random_problem, tensor_cuts
from mlp_reference import point_reference

pytestmark = pytest.mark.gpu

FAMILY = 'dw_last_job'
# (depth, width, Stokes planes): the four forms at width 256, one of them again at four planes, and the same job on the 4 x 2 grid
CASES = [(3, 256, 0), (4, 256, 0), (5, 256, 0), (6, 256, 0), (4, 256, 4), (6, 128, 0)]
_PROBLEMS = {}


def problem(depth, width, S):
    """random_problem (with its float64 reference) of a case, made once."""
    key = (depth, width, S)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = random_problem(width, depth, S, 3)
    return _PROBLEMS[key]


def upstream_gradient(prob):
    """(B, Sx, R) float64 of f32-rounded values, different in every frame and plane."""
    H, Wd, _, B = RANDOM_PROBLEM_SHAPE
    gen = torch.Generator().manual_seed(17 + prob['S'])
    return (torch.rand((B, max(prob['S'], 1), H * Wd), generator=gen, dtype=torch.float64) - 0.4).float().double()


def stokes_weights(prob):
    """J of the problem as mlp_reference.Reference takes it: (Sx, H, W, G), ones for a problem without Stokes factors."""
    g = prob['g']
    return torch.tensor(np.asarray(g['J'], dtype=np.float64)) if prob['S'] else torch.ones((1,) + g['coords'].shape[1:], dtype=torch.float64)


def tape_route(dev, name, prob, recipe, drop=None):
    """render_train + render_bwd_tape of a case on a fresh predictor -> (images (B, Sx, R), flat gradient) as float32 arrays."""
    pred, eng, geom, flat, tM0 = device_setup(prob['g'], 'bf16', dev, drop=drop)
    flags, _ = assert_path(name, eng, geom, 'bf16', recipe, False, compact=True)
    assert flags['drop_ga'] and not flags['fused128'], (name, flags)          # the output layer rides on the layer depth-1 job
    eng.pack(flat)
    images = eng.render_train(geom, tM0).clone()
    dimg = upstream_gradient(prob).float().to(dev).contiguous()
    assert tuple(dimg.shape) == (len(prob['t_frames']), geom.Sx, geom.R)
    grad = eng.render_bwd_tape(geom, tM0, dimg).clone()
    groups = (geom.P_eff + 31) // 32
    return images.cpu().numpy(), grad.cpu().numpy(), (geom.P_eff, groups)


def emulator_figures(dev, name, prob, recipe, drop=None):
    """The recorded-tape route against the emulator of `recipe` (without the ray samples `drop`) -> (figures, whether two runs on
    fresh predictors agreed bit for bit, the reference)."""
    ref = point_reference(FAMILY, name, prob, recipe, drop)
    J = stokes_weights(prob)
    B, Sx = len(prob['t_frames']), J.shape[0]
    img_ref = ref.images(J).numpy().reshape(B, Sx, -1)
    gref = ref.grad(upstream_gradient(prob), J)
    images, grad, (P_eff, groups) = tape_route(dev, name, prob, recipe, drop)
    images2, grad2, _ = tape_route(dev, name, prob, recipe, drop)
    repro = first_difference(grad, grad2) is None and first_difference(images, images2) is None
    assert np.abs(img_ref).max() > 0 and np.abs(gref).max() > 0
    cuts = tensor_cuts(prob['g'])
    fig = dict(image=maxerr(images.astype(np.float64).reshape(img_ref.shape), img_ref), grad=l2err(grad.astype(np.float64), gref),
               tensor=max(tensor_l2(grad.astype(np.float64), gref, cuts, True)))
    print('\n[dW last job] %-12s %-9s points per frame %d = %d groups (last: %d points)  image %.2e  grad L2 %.2e  worst tensor %.2e  '
          'repeat bitwise %s%s' % (name, recipe, P_eff, groups, P_eff - 32 * (groups - 1), fig['image'], fig['grad'], fig['tensor'], repro,
                                   '' if drop is None else '  [tied samples taken out]'))
    return fig, repro, ref


@pytest.mark.parametrize('depth,width,S', CASES, ids=['%dx%d S%d' % c for c in CASES])
def test_last_job_forms(dev, depth, width, S):
    """The four forms of the layer depth-1 job at width 256 (8 x 1 wave grid), one at four Stokes planes, and depth 6 at width 128 (the
    untouched 4 x 2 grid): chi^2 step against the float64 oracle, recorded-tape route against the emulator, twice, bit for bit."""
    name = '%dx%d S%d' % (depth, width, S)
    prob = problem(depth, width, S)
    assert RANDOM_PROBLEM_DOMAIN == SHELL and prob['g']['coords'].shape[1:] == RANDOM_PROBLEM_SHAPE[:3]
    recipe = expected_recipe(depth, kernel_width(width), False)
    assert recipe == ('ga0_chain' if width == 256 else 'fold')
    # (1) the chi^2 step against the float64 oracle, under the bounds of test_random_problem_f32_and_bf16
    ierr, gerr, l2 = random_problem_errors(prob, 'bf16', dev)
    print('\n[dW last job] %-12s float64 oracle: image %.2e  gradient max %.2e  L2 %.2e' % (name, ierr, gerr, l2))
    assert ierr < IMG_TOL['bf16'], (name, ierr)
    assert gerr < GTOL['bf16'] and l2 < L2TOL['bf16'], (name, gerr, l2)
    # (2) the recorded-tape route against the emulator, under the caps of class 'random'
    caps = CAPS['random']
    fig, repro, ref = emulator_figures(dev, name, prob, recipe)
    ok, _ = held_or_adjudicated(name, (fig, repro), lambda run: all(run[0][k] < caps[k] for k in caps), lambda: ref.relu_ties(prob['g']),
                                lambda ties: emulator_figures(dev, name, prob, recipe, drop=ties)[:2], lambda run: run[1])
    assert ok, (name, fig, caps)
    assert repro, (name, 'two runs differ')


def test_two_frame_groups_equal_one(dev):
    """The layer depth-1 job adding into its slabs (BwdArgs::accumulate = 1, the second frame group of a step): depth 3 at width 256
    (both skip forms: the output row, its encoded-input part and its bias all add into what the first group left) on
    frame_chunk_cases.build_problem's draw of the ragged grid, three frames in groups of 2 + 1 against all three at once, under the
    rule of test_gpu_backward.test_frame_group_taped_step_equals_full_step."""
    from bhnerf_amd import _hip, network, units
    H, Wd, G, B = RANDOM_PROBLEM_SHAPE
    depth, width, cap = 3, 256, 2
    g = build_problem(depth, width, 'bf16', 0, 3, H, Wd, G, SHELL, B)['g']
    rng = np.random.default_rng(3)
    shape = (B, H, Wd)
    tg = dict(target=rng.uniform(0, 1e-2, shape), sigma=rng.uniform(0.5, 2.0, shape), offset=np.zeros(shape))
    res = []
    for cap_frames in (None, cap):
        pred, rt = predictor_of(g, 'bf16', dev), ray_args(g)
        eng = pred.engine()
        if cap_frames is not None:      # cap = tape of exactly `cap` frames
            geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], None, rt['g'], rt['dtau'], rt['Sigma'])
            eng.max_workspace_bytes = int(_hip.lib().bhn_render_bwd_workspace_bytes(C.byref(eng.model), eng.mode, cap_frames, geom.P_eff,
                                                                                      dev.index or 0))
            assert not eng.fits_tape(B, geom.P_eff) and eng.tape_group(B, geom.P_eff) == cap_frames
            flags = eng.tape_info((geom.P_eff + 31) // 32)['flags']
            assert not flags['general'] and flags['ga0_chain'] and flags['drop_ga'] and not flags['fused128'], flags
        tree0 = golden_tree(g)
        state = pred.init_state(network.ParamTree(tree0), num_iters=2, lr_init=1e-3, lr_final=1e-4)
        for _ in range(2):
            loss, state, images = network.gradient_step_image(
                state, units.hr, 'full', tg['target'], tg['sigma'], tg['offset'], g['t_frames'], rt['coords'], rt['Omega'],
                rt['J'], rt['g'], rt['dtau'], rt['Sigma'], rt['t_start_obs'], rt['t_geos'], rt['t_injection'], 1.0)
        res.append((loss.item(), images.clone(), state.flat.clone()))
    (l0, i0, p0), (l1, i1, p1) = res
    start = pred.engine().flatten(tree0)
    moved = float((p0 - start).abs().max())
    print('\n[dW last job] frame groups 3x256: loss %.3e (rel. diff %.1e)  images max diff / max %.1e  parameters max diff %.1e, moved %.1e'
          % (l0, abs(l0 - l1) / abs(l0), float((i0 - i1).abs().max() / i0.abs().max()), float((p0 - p1).abs().max()), moved))
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    assert torch.allclose(i0, i1, rtol=1e-5, atol=1e-6 * float(i0.abs().max()))
    # Adam normalises the step, so parameters move ~lr per step; compare against the total movement
    assert moved > 1e-4 and float((p0 - p1).abs().max()) < 2e-2 * moved
