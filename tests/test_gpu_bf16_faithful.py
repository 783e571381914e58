"""GPU tests of the bf16 mode against the rounding-faithful emulator (oracle/oracle_bf16.py), next to the float64 comparisons of
test_gpu_backward.py / test_gpu_forward.py / test_gpu_fullsize*.py (which stay as they are).

The float64 oracle can only hold the bf16 kernels to the bf16 QUANTISATION noise (gradient L2 2e-2 ... 6e-2): a kernel a few
per cent wrong passes it.  The emulator rounds every MFMA operand to bf16 where the kernels round it, per path (its RECIPES:
generic tape backward, W_out fold / drop_ga, ga0_chain, fused 4x128, general path), so what is left is the kernels' f32
accumulation order and the rare bf16 rounding that order flips.  Every case checks that the library takes the path whose
recipe it is compared with (gpu_support.assert_path), then compares images and the chi^2 loss and gradient
(network.loss_fn_image), the emission (bhn_predict_fwd) and the gradient of a random upstream image gradient through BOTH
backward routes (render_train + render_bwd_tape, and the recompute route render_bwd).

Tolerances: per case 4x the figures observed on the MI355X (OBSERVED: image error / maximum, emission relative L2, loss relative
error, gradient relative L2 -- the worst of the three routes -- and the worst relative L2 of one kernel / bias tensor; the kernels
are bitwise reproducible), capped at the required bounds (CAPS: 20x under the float64 comparisons; the per-tensor figure at 2x the
gradient cap).  Worst observed: goldens
1.1e-7 gradient / 3.9e-7 images (f64: 6e-2 / 1e-2); fused 4x128 3.5e-5 / 2.1e-4; config 2 subset 6.6e-5, config 5 subset 5.6e-5
(f64: 2e-2, 3e-2); random and general-path problems up to 2.2e-3 (most <= 2e-4); eight hidden layers at width >= 256 up to
3.1e-3 (class 'deep', not capped: rounding flips compound down eight layers, not ties; every case prints its per-layer error
profile, and the float32-accumulating emulator reproduces the profile and the size on CPU).  Mutants of the emulator: every case
must see the ones required_mutants names at >= 5x its bounds (the goldens and random problems in tests/test_oracle_bf16_cpu.py,
the fused 4x128 and config 2 / 5 cases here, sharing the emulator's forward); which ones are not required, and why, is stated there.  ReLU ties are the f32 mode's: bf16 keeps f32's
exponent range, so a relu decision flips only where the f32 accumulation flips it; they are detected on the EMULATOR's forward
(mlp_reference.tie_points: the bf16 network's pre-activations, not the float64 one's) and adjudicated by
mlp_bounds.held_or_adjudicated.
"""
import numpy as np
import pytest
import torch

from conftest import golden_tree
from buffer_contract_cases import RAY_SETS
from frame_chunk_cases import build_problem
from gpu_support import assert_path, chi2_step, dev, device_setup, problem_of, ray_args  # noqa: F401
from mlp_bounds import (FIELDS, GENERAL_SHAPES, LAST_JOB_SHAPES, RANDOM_SHAPES, bounds, check_mutants, expected_recipe, held_or_adjudicated, kernel_width,
                        l2err as l2, maxerr as mx, mutant_ratios, problem_class, tensor_l2)
from mlp_problems import (CONFIG2, CONFIG2_DOMAINS, config_problem, f32r, oracle_inputs_of, random_problem_inputs, ray_subset,
                          rays_through_domain, stokes_domain, stokes_problem, t64, targets, tensor_cuts, without_samples)
from mlp_reference import tie_points
from oracle import oracle_bf16 as ob
from oracle import oracle_np as onp
from oracle import oracle_torch as ot

pytestmark = pytest.mark.gpu

# The figures observed on the MI355X per case (OBSERVED), the caps of each class (CAPS), the bound rule, the mutant requirements and the
# shape lists live in tests/mlp_bounds.py: tests/test_oracle_bf16_cpu.py reads them too.


def check_case(name, dev, tree, geo, t_frames, t_inj, dom, depth, width, deg, target, sigma, offset, dt='full', loss_scale=1.0,
               do_skip=True, general=False, dimg_seed=0, compact=None, drop=None, mutant_cls=None):
    """Device (bf16) vs emulator on one problem: geo holds float64 arrays of f32-rounded values (coords (3,H,W,G), Omega, t_geos,
    g, dtau, Sigma, J (S,H,W,G) or None); `drop` (H,W,G) bool: ray samples taken out of the problem (Doppler weight g = 0 on
    both sides: the relu-tie adjudication).  Returns (errors, recipe, the emulator's tied ray samples)."""
    geo = without_samples(geo, drop)
    J = geo.get('J')
    S = 0 if J is None else J.shape[0]
    g = problem_of(tree, geo, t_frames, t_inj, dom, deg, depth, width)
    pred, eng, geom, flat, tM0 = device_setup(g, 'bf16', dev, do_skip=do_skip)
    recipe = expected_recipe(depth, kernel_width(width), general)
    assert_path(name, eng, geom, 'bf16', recipe, general, compact=compact)
    # the emulator
    ks, bs, geom_t, hp = oracle_inputs_of(tree, geo, t_inj, dom, deg, depth, do_skip=do_skip)
    em = ob.Bf16Trainer(ks, bs, geom_t, hp, recipe)
    cuts = tensor_cuts(g, depth)
    if mutant_cls is not None:            # (the mutants share the faithful forward: loss_and_grad_variants)
        variants = em.loss_and_grad_variants(t64(t_frames), t64(target), t64(sigma), t64(offset), loss_scale, dt)
        check_mutants(name, mutant_cls, mutant_ratios(variants, bounds(name, mutant_cls, deg), cuts))
        loss_ref, img_ref, grads_ref = variants[None]
    else:
        loss_ref, img_ref, grads_ref = em.loss_and_grad(t64(t_frames), t64(target), t64(sigma), t64(offset), loss_scale, dt)
    gref = ob.flat(grads_ref)
    img_ref = img_ref.numpy()
    # (1) the chi^2 step through the reference-shaped API
    def sq(v):          # the reference-shaped API squeezes singleton axes: the plane axis of S = 1, a ray grid of one row or column
        v = v[:, 0] if S == 1 else v
        return v.reshape(v.shape[:-2] + tuple(n for n in v.shape[-2:] if n != 1)) if dt == 'full' else v
    loss, images, gdev = chi2_step(pred, flat, ray_args(g), t_frames, sq(target), sq(sigma), sq(offset), loss_scale, dt)
    img = images.cpu().numpy().reshape(img_ref.shape)
    gdev = gdev.astype(np.float64)
    assert np.abs(img_ref).max() > 0 and np.abs(gref).max() > 0
    # (2) emission: bhn_predict_fwd
    eng.pack(eng.flatten(tree))
    emis = eng.predict(geom, tM0).cpu().numpy().reshape(len(t_frames), -1)
    emis_ref = em.emission(t64(t_frames)).numpy().reshape(emis.shape)
    # (3) both backward routes on a random upstream image gradient
    gen = torch.Generator().manual_seed(dimg_seed)
    dimg = (torch.rand((len(t_frames), geom.Sx, geom.R), generator=gen, dtype=torch.float64) - 0.4)
    eng.render_train(geom, tM0)
    g_tape = eng.render_bwd_tape(geom, tM0, dimg.float().to(dev)).cpu().numpy().astype(np.float64)
    g_rec = eng.render_bwd(geom, tM0, dimg.float().to(dev)).cpu().numpy().astype(np.float64)
    d_em = dimg.float().double().reshape((len(t_frames), geom.Sx) + tuple(img_ref.shape[-2:]))
    if S == 0:
        d_em = d_em[:, 0]
    glin = ob.flat(em.grad_linear(t64(t_frames), d_em))
    # per parameter tensor (kernel_l, bias_l in flax order): the largest relative L2 error of any of them on any route
    tens = max(max(tensor_l2(a, b, cuts, True)) for a, b in ((gdev, gref), (g_tape, glin), (g_rec, glin)))
    ties = tie_points(geo, em, t64(t_frames))
    r = dict(image=mx(img, img_ref), emission=l2(emis, emis_ref), loss=abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()),
             grad=max(l2(gdev, gref), l2(g_tape, glin), l2(g_rec, glin)), tensor=tens)
    print('\n[bf16 vs emulator] %-34s %-9s image %.2e  emission %.2e  loss %.2e  grad L2 %.2e (chi2 %.2e tape %.2e recompute %.2e)  '
          'worst tensor %.2e  tied samples %d' % (name, recipe, r['image'], r['emission'], r['loss'], r['grad'], l2(gdev, gref),
                                                  l2(g_tape, glin), l2(g_rec, glin), tens, int(ties.sum())))
    # per-layer profile (recorded-tape route): relative L2 of dK_l, l = 0 .. depth -- where along the chain the difference grows
    print('    per-layer dK L2 (layer 0 .. output): ' + ' '.join('%.1e' % l2(g_tape[cuts[2 * i]:cuts[2 * i + 1]], glin[cuts[2 * i]:cuts[2 * i + 1]])
                                                            for i in range(depth + 1)))
    return r, recipe, ties


def check_and_adjudicate(name, cls, deg, run):
    """run(drop) -> check_case's result.  Bounds of class `cls`; where they are missed and the emulator's forward has relu ties
    (conftest.relu_tie_count's criterion on the bf16 forward), the same problem without exactly the tied ray samples must meet
    them -- otherwise the difference was not a tie and the test fails."""
    b = bounds(name, cls, deg)
    r, recipe, ties = run(None)
    ok, r2 = held_or_adjudicated(name, r, lambda r: all(r[k] < b[k] for k in FIELDS), lambda: ties, lambda ties: run(ties)[0])
    assert ok or r2 is not None, (name, cls, r, b)
    assert ok, (name, 'NOT a tie: without the %d tied samples' % int(ties.sum()), r2, 'before', r, b)
    return r if r2 is None else r2


def random_case(width, depth, S, deg):
    prob = random_problem_inputs(width, depth, S, deg)
    g = prob['g']
    geo = {k: g[k] for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    geo['J'] = g['J'] if S else None
    return prob, geo, golden_tree(g)


@pytest.mark.parametrize('width,depth,S,deg', RANDOM_SHAPES + GENERAL_SHAPES)
def test_random_problems_against_emulator(dev, width, depth, S, deg):
    """test_random_problem_f32_and_bf16's problems (widths 20..256 zero-padded, depths 2..8, S 0..3, posenc 0..4, G = 50 rays
    across wave tiles, a point-compacted domain) and test_shapes_outside_the_fused_kernels' general-path shapes."""
    general = width > 256 or deg > 4
    prob, geo, tree = random_case(width, depth, S, deg)
    name = '%dx%d S%d deg%d' % (depth, width, S, deg)
    check_and_adjudicate(name, problem_class(depth, width), deg, lambda drop: check_case(
        name, dev, tree, geo, prob['t_frames'], prob['t_inj'], tuple(prob['g']['hparams'][:4]), depth, width, deg, prob['target'],
        prob['sigma'], prob['offset'], general=general, compact=True, drop=drop))


def last_job_case(depth, width):
    """(name, check_case's arguments from `tree` to `offset`) of a LAST_JOB_SHAPES problem: buffer_contract_cases' ragged ray set
    (37 rays x 50 samples = 58 groups, the last one 26 points), three frames, S = 2, posenc degree 3."""
    H, Wd, G, dom = RAY_SETS['ragged']
    g = build_problem(depth, width, 'bf16', 2, 3, H, Wd, G, dom, 3)['g']
    geo = {k: g[k] for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma', 'J')}
    rng = np.random.default_rng(500 + 7 * width + depth)
    tshape = (3, 2, H, Wd)
    target = rng.uniform(0, 1e-3, tshape); sigma = rng.uniform(0.5, 2.0, tshape); offset = np.zeros(tshape)
    return '%dx%d S2 ragged' % (depth, width), (golden_tree(g), geo, g['t_frames'], float(g['t_injection']), dom, depth, width, 3, target,
                                                 sigma, offset)


@pytest.mark.parametrize('depth,width', LAST_JOB_SHAPES)
def test_last_job_forms_against_emulator(dev, depth, width):
    """The forms of the dW kernel's layer depth-1 job (dw_body2 LAST: gA_{depth-1} rebuilt from h_depth, the output layer's row) that
    no other case runs at their kernel width -- depth 3 (skip-concat into layer 2 and into the output layer) at widths 64, 128, 256 and
    depth 5 (into the output layer only) at width 32 -- on a dense ragged ray set.  check_case asserts the path: drop_ga, not fused128."""
    name, args = last_job_case(depth, width)
    check_and_adjudicate(name, 'random', 3, lambda drop: check_case(name, dev, *args, compact=False, drop=drop))


@pytest.mark.parametrize('dt', ['full', 'lc'])
@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e', 'f'])
def test_goldens_against_emulator(dev, golden, tag, dt):
    g = golden('g5_predict_' + tag)
    hp = g['hparams']
    geo = {k: f32r(g[k]) for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    geo['J'] = f32r(g['J']) if g['J'].ndim else None
    tree = golden_tree({k: (f32r(v) if k.startswith(('kernel', 'bias')) else v) for k, v in g.items()})
    tg = targets(g, dt)
    name = 'g5_%s %s' % (tag, dt)
    check_and_adjudicate(name, 'golden', int(hp[4]), lambda drop: check_case(
        name, dev, tree, geo, g['t_frames'], float(g['t_injection']), tuple(hp[:4]), int(hp[5]), int(hp[6]), int(hp[4]),
        tg['target'], tg['sigma'], tg['offset'], dt=dt, loss_scale=float(hp[7]), drop=drop))


@pytest.mark.parametrize('rows', [48, 47])
@pytest.mark.parametrize('width,do_skip', [(128, True), (128, False), (113, True), (113, False), (97, True), (97, False)])
def test_fused_4x128_against_emulator(dev, rows, width, do_skip):
    """bwd128_kernel + reduce128_kernel (output row from the un-folded gradient of layer 3) at widths 97 / 113 / 128, with and
    without the skip connection, on both sides of the 8 / 12-group tile threshold of the forward pair (test_gpu_backward.py
    test_reference_default_network_on_twelve_and_eight_group_tiles): all-active dense domain."""
    from bhnerf_amd import synthetic
    H, Wd, G, B = rows, 32, 64, 2
    geo = synthetic.synthetic_geodesics(H, Wd, G, fov_M=16.0, inc_deg=60.0, seed=7)
    t_inj = float(geo['t_injection'])
    geo = {k: f32r(geo[k]) for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    geo['J'] = None
    rng = np.random.default_rng(21 + width)
    tree = onp.he_uniform_params(rng, 4, width, 21, do_skip=do_skip, dtype=np.float32)
    for i in range(5):
        d = tree['MLP_0']['Dense_%d' % i]
        d['kernel'] = f32r(d['kernel']); d['bias'] = f32r(rng.uniform(-0.05, 0.05, d['bias'].shape))
    tree['MLP_0']['Dense_4']['bias'] = tree['MLP_0']['Dense_4']['bias'] + 9.0
    target = rng.uniform(0, 1e-2, (B, H, Wd)); sigma = rng.uniform(0.5, 2.0, (B, H, Wd)); offset = np.zeros((B, H, Wd))
    name = '4x%d rows %d skip %d' % (width, rows, do_skip)
    check_and_adjudicate(name, 'fused128', 3, lambda drop: check_case(
        name, dev, tree, geo, np.array([0.1, 0.6]), t_inj, (8.0, 0.0, np.inf, np.inf), 4, width, 3, target, sigma, offset,
        do_skip=do_skip, compact=False, drop=drop, mutant_cls=None if drop is not None else 'fused128'))


@pytest.mark.parametrize('domain', ['masked', 'all_active'])
def test_config2_ray_subset_against_emulator(dev, domain):
    """The headline path (4x256, ga0_chain): config 2's geometry and weights (test_gpu_fullsize.py), 256 rays x 64 samples x
    8 frames."""
    c = CONFIG2
    p = config_problem(**c)
    geo, tree, t_frames, B = p['geo'], p['tree'], p['t_frames'], len(p['t_frames'])
    rays = np.sort(np.random.default_rng(12).choice(c['H'] * c['W'], size=256, replace=False))
    sgeo = {k: (None if v is None else f32r(v)) for k, v in ray_subset(geo, rays).items()}
    rng = np.random.default_rng(13)
    target = rng.uniform(0, 1e-2, (B, 16, 16)); sigma = rng.uniform(0.5, 2.0, (B, 16, 16)); offset = np.zeros((B, 16, 16))
    name = 'config 2 subset %s' % domain
    check_and_adjudicate(name, 'subset', 3, lambda drop: check_case(
        name, dev, tree, sgeo, t_frames, float(geo['t_injection']), CONFIG2_DOMAINS[domain], 4, 256, 3, target, sigma, offset,
        compact=(domain == 'masked'), drop=drop, mutant_cls=None if drop is not None else 'subset'))


def test_config5_ray_subset_lc_stokes_against_emulator(dev):
    """Config 5 (4x128, fused backward) 'lc' chi^2 of the three Stokes light curves on the 256 rays of
    test_gpu_fullsize_stokes.py's gradient test (point-compacted domain, S = 3)."""
    p = stokes_problem('config5')
    c, geo = p['c'], p['geo']
    sgeo = {k: f32r(v) for k, v in ray_subset(geo, rays_through_domain(geo, c, 41), stokes=True).items()}
    # the light curves of the subset -> test_gpu_fullsize_stokes' well-conditioned chi^2 (residual >= 40 %, one noise level)
    tr = ot.CpuTrainer(*oracle_inputs_of(p['tree'], sgeo, geo['t_injection'], stokes_domain(c), 3, 4, GM_c3=p['GM_c3']))
    lc0 = tr.forward(t64(p['t_frames'])).detach().sum(dim=(-1, -2)).numpy()
    rng = np.random.default_rng(42)
    target = lc0 * rng.uniform(0.3, 0.6, lc0.shape)
    sigma = np.abs(lc0[:, :1]).mean() * rng.uniform(0.05, 0.2, lc0.shape)
    offset = np.zeros_like(lc0)
    name = 'config 5 subset lc S3'
    check_and_adjudicate(name, 'subset', 3, lambda drop: check_case(
        name, dev, p['tree'], sgeo, p['t_frames'], float(geo['t_injection']), stokes_domain(c), 4, 128, 3,
        target, sigma, offset, dt='lc', compact=True, drop=drop, mutant_cls=None if drop is not None else 'subset'))
