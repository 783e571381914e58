"""CPU tests of the rounding-faithful bf16 emulator (oracle/oracle_bf16.py), the reference the GPU suite holds the bf16 kernels to
(tests/test_gpu_bf16_faithful.py):

* its rounding helper is bit for bit torch's float32 -> bfloat16 (round to nearest even) and its relu is the kernels' (round,
  then clamp: -0 -> +0, a bf16 +0 is inactive);
* with the rounding switched off, every recipe IS the float64 model of oracle_torch (forward, loss and autograd gradient to
  1e-12): the W_out fold and the fused 4x128 output row sum_k K G + b g are algebraically the plain backward;
* the mutants of the emulator (one 32-point group dropped from every dW, the output bias gradient scaled by 1 + 2^-8,
  activations truncated instead of rounded, dout not rounded) that mlp_bounds.required_mutants names move the goldens
  and the random / general-path problems of the GPU tests by at least 5x each case's GPU bound (the fused 4x128 and config 2 / 5
  cases check theirs in the GPU test itself);
* the largest GPU errors are what float32 accumulation alone does to those problems (accum32), not a missing rounding point.
"""
import numpy as np
import pytest
import torch

from mlp_bounds import (GENERAL_SHAPES, OBSERVED, RANDOM_SHAPES, bounds, check_mutants, expected_recipe, kernel_width, mutant_ratios,
                        problem_class)
from mlp_problems import golden_problem, random_problem_emulator_args, small_problem
from oracle import oracle_bf16 as ob
from oracle import oracle_torch as ot

PRED = ['a', 'b', 'c', 'd', 'e', 'f']


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def torch_bf16_bits(f32):
    return torch.from_numpy(np.ascontiguousarray(f32, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


# --------------------------------------------------------------------------------------------------------------------------
# rounding
# --------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_bit_exact_on_random_patterns():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 2 ** 32, size=1_200_000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000][:1_000_000]            # finite f32 bit patterns
    assert len(u) == 1_000_000
    f = u.view(np.float32)
    assert np.array_equal(ob.bf16_bits(f), torch_bf16_bits(f))
    # the float64 entry point: rounds the f32 value (the kernels hold f32), returns the bf16 value exactly
    r = ob.round_bf16(f.astype(np.float64))
    assert np.array_equal(r.astype(np.float32).view(np.uint32) & 0xFFFF, np.zeros(len(u), np.uint32))
    assert np.array_equal(ob.bf16_bits(r.astype(np.float32)), torch_bf16_bits(f))


def test_bf16_rounding_hand_cases():
    cases = {
        0x3F808000: 0x3F80,   # 1 + 2^-8: a tie, even neighbour below -> down
        0x3F818000: 0x3F82,   # 1 + 3 * 2^-8: a tie, odd below -> up
        0xBF808000: 0xBF80,   # negative ties, both directions
        0xBF818000: 0xBF82,
        0x3F808001: 0x3F81,   # just above a tie -> up
        0x3F807FFF: 0x3F80,   # just below -> down
        0x00000000: 0x0000,   # +0
        0x80000000: 0x8000,   # -0 keeps its sign
        0x00000001: 0x0000,   # smallest subnormal -> +0
        0x00008000: 0x0000,   # subnormal tie to even (0)
        0x00018000: 0x0002,   # subnormal tie, odd below -> up
        0x807FFFFF: 0x8080,   # largest negative subnormal -> the smallest normal
        0x7F7F7FFF: 0x7F7F,   # largest finite bf16
        0x7F7F8000: 0x7F80,   # a tie above it, odd below -> inf (round to nearest even)
        0x7F7FFFFF: 0x7F80,   # largest finite f32 -> inf
        0xFF7FFFFF: 0xFF80,
    }
    u = np.array(list(cases), dtype=np.uint32)
    want = np.array(list(cases.values()), dtype=np.uint16)
    got = ob.bf16_bits(u.view(np.float32))
    assert np.array_equal(got, want), [(hex(a), hex(b), hex(c)) for a, b, c in zip(u, got, want) if b != c]
    assert np.array_equal(torch_bf16_bits(u.view(np.float32)), want)
    # truncation (the mutant) drops the low half
    assert ob.round_bf16(np.float64(np.uint32(0x3F818000).view(np.float32)), 'trunc') == np.uint32(0x3F810000).view(np.float32)


def test_relu_rounds_then_clamps():
    a = torch.tensor([-0.0, -1e-40, -3.0, 0.0, 1e-45, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 2.5], dtype=torch.float64)
    h, on = ob.relu_bf16(a, 'round_clamp')
    assert not np.signbit(h.numpy()).any()                                  # -0 -> +0, negatives -> +0
    assert h.tolist()[:5] == [0.0] * 5 and h.tolist()[5:] == [1.0, 1.0 + 4 * 2 ** -8, 2.5]
    assert on.tolist() == [False] * 5 + [True] * 3                          # a bf16 +0 (1e-45 rounds to it) is inactive
    h2, on2 = ob.relu_bf16(a, 'clamp_round')
    assert torch.equal(h2, h) and torch.equal(on2, on)
    ht, _ = ob.relu_bf16(torch.tensor([1.0 + 3 * 2 ** -8], dtype=torch.float64), 'round_clamp', 'trunc')
    assert ht.item() == 1.0 + 2 * 2 ** -8


# --------------------------------------------------------------------------------------------------------------------------
# problems
# --------------------------------------------------------------------------------------------------------------------------
def identity_check(ks, bs, geom, hp, tf, tg, scale, dt):
    l0, i0, g0 = ot.CpuTrainer(ks, bs, geom, hp).loss_and_grad(tf, *tg, scale, dt)
    g0 = torch.cat([g.reshape(-1) for g in g0]).numpy()
    assert np.abs(g0).max() > 0 and float(i0.abs().max()) > 0
    for recipe in ob.RECIPES:
        em = ob.Bf16Trainer(ks, bs, geom, hp, recipe, rounding=False)
        l1, i1, g1 = em.loss_and_grad(tf, *tg, scale, dt)
        g1 = torch.cat([g.reshape(-1) for g in g1]).numpy()
        assert rel(i1, i0) < 1e-12 and abs(l1.item() - l0.item()) <= 1e-12 * abs(l0.item()), recipe
        assert rel(g1, g0) < 1e-12, (recipe, rel(g1, g0))
        e0 = ot.predictor(ks, bs, tf, geom['coords'], geom['Omega'], geom['t_start_obs'], geom['t_geos'], geom['t_injection'], hp['GM_c3'],
                          hp['scale'], hp['rmin'], hp['rmax'], hp['z_width'], hp['posenc_deg'], hp['net_depth'], hp.get('do_skip', True))
        assert rel(em.emission(tf), e0.detach()) < 1e-12
        # ... and rounding ON moves all of them by the bf16 quantisation (the switch does something)
        l2_, _, g2 = ob.Bf16Trainer(ks, bs, geom, hp, recipe).loss_and_grad(tf, *tg, scale, dt)
        assert rel(torch.cat([g.reshape(-1) for g in g2]).numpy(), g0) > 1e-4, recipe


@pytest.mark.parametrize('dt', ['full', 'lc'])
@pytest.mark.parametrize('tag', PRED)
def test_rounding_off_is_the_f64_model_on_goldens(golden, tag, dt):
    ks, bs, geom, hp, tf, tg, scale = golden_problem(golden('g5_predict_' + tag), dt)
    identity_check(ks, bs, geom, hp, tf, tg, scale, dt)


@pytest.mark.parametrize('depth,S,do_skip', [(2, 0, True), (2, 1, False), (3, 3, True), (3, 0, False), (4, 1, True), (4, 3, False),
                                             (8, 0, True), (8, 3, False), (5, 1, True)])
@pytest.mark.parametrize('dt', ['full', 'lc'])
def test_rounding_off_is_the_f64_model_on_random_networks(depth, S, do_skip, dt):
    ks, bs, geom, hp, tf, tg = small_problem(depth, 48, S, do_skip)
    if dt == 'lc':
        tg = [v.sum(dim=(-1, -2)) for v in tg]
    identity_check(ks, bs, geom, hp, tf, tg, 1.0, dt)


def test_recipe_selection_names_every_path():
    assert ob.recipe_for({'general': True, 'drop_ga': False}) == 'general'
    assert ob.recipe_for({'fused128': True, 'drop_ga': True}) == 'fused128'
    assert ob.recipe_for({'ga0_chain': True, 'drop_ga': True}) == 'ga0_chain'
    assert ob.recipe_for({'drop_ga': True}) == 'fold'
    assert ob.recipe_for({'drop_ga': False}) == 'generic'
    with pytest.raises(ValueError):
        ob.Bf16Trainer([], [], {}, dict(net_depth=0), recipe='nope')


# --------------------------------------------------------------------------------------------------------------------------
# mutants: distances on the GPU tests' problems
# --------------------------------------------------------------------------------------------------------------------------
def gpu_cases(golden):
    """(name, bound class, posenc degree, emulator arguments, recipe) of the goldens and the random / general-path problems of
    test_gpu_bf16_faithful (its fused 4x128 and config 2 / 5 cases check their mutants themselves: check_case(mutant_cls=...))."""
    for tag in PRED:
        g = golden('g5_predict_' + tag)
        for dt in ('full', 'lc'):
            ks, bs, geom, hp, tf, tg, scale = golden_problem(g, dt)
            yield ('g5_%s %s' % (tag, dt), 'golden', hp['posenc_deg'], (ks, bs, geom, hp, tf, tg, scale, dt),
                   expected_recipe(hp['net_depth'], kernel_width(int(g['hparams'][6])), False))
    for (w, d, S, deg) in RANDOM_SHAPES + GENERAL_SHAPES:
        ks, bs, geom, hp, tf, tg = random_problem_emulator_args(w, d, S, deg)
        yield ('%dx%d S%d deg%d' % (d, w, S, deg), problem_class(d, w), deg, (ks, bs, geom, hp, tf, tg, 1.0, 'full'),
               expected_recipe(d, kernel_width(w), w > 256 or deg > 4))


def test_mutants_are_visible_to_the_gpu_bounds(golden):
    """On every golden and random / general-path problem of the GPU tests the mutants mlp_bounds.required_mutants names
    move the problem by >= 5x that case's GPU bound in at least one bounded figure (gradient L2, one tensor, images); every
    distance is printed.  (bias_scale and dout_unrounded are required on the goldens only: see test_gpu_bf16_faithful.)"""
    for name, cls, deg, (ks, bs, geom, hp, tf, tg, scale, dt), recipe in gpu_cases(golden):
        variants = ob.Bf16Trainer(ks, bs, geom, hp, recipe).loss_and_grad_variants(tf, *tg, scale, dt)
        cuts = np.cumsum([0] + [t.numel() for k, b in zip(ks, bs) for t in (k, b)])
        check_mutants(name, cls, mutant_ratios(variants, bounds(name, cls, deg), cuts))


# the cases whose GPU errors stand out (gradient L2 >= 5e-4 against the emulator: up to 50x the same path's other problems)
LARGEST = [(256, 4, 3, 1), (256, 8, 0, 3), (256, 8, 3, 3), (384, 8, 2, 4), (512, 8, 0, 8)]


def test_accumulation_noise_explains_the_largest_errors():
    """The GPU errors of LARGEST are the kernels' f32 accumulation, not a missing rounding point: the emulator with float32 instead
    of float64 accumulation (accum32 -- same rounding points, another accumulation) moves each of them by >= 1/8 of what the GPU is
    observed at (OBSERVED), and by >= 10x what it moves the quiet 4x256 S0 problem of the same path; its per-layer profile grows
    towards layer 0 as the GPU's does (printed)."""
    def acc32(w, d, S, deg):
        ks, bs, geom, hp, tf, tg = random_problem_emulator_args(w, d, S, deg)
        recipe = expected_recipe(d, kernel_width(w), w > 256 or deg > 4)
        _, _, g0 = ob.Bf16Trainer(ks, bs, geom, hp, recipe).loss_and_grad(tf, *tg, 1.0, 'full')
        _, _, g1 = ob.Bf16Trainer(ks, bs, geom, hp, recipe, accum32=True).loss_and_grad(tf, *tg, 1.0, 'full')
        prof = [rel(a.numpy(), b.numpy()) for a, b in zip(g1[:d + 1], g0[:d + 1])]
        return rel(ob.flat(g1), ob.flat(g0)), prof
    quiet, _ = acc32(256, 4, 0, 3)
    for (w, d, S, deg) in LARGEST:
        name = '%dx%d S%d deg%d' % (d, w, S, deg)
        dist, prof = acc32(w, d, S, deg)
        print('accum32 %-14s %.2e (GPU %.1e)  per-layer dK %s' % (name, dist, OBSERVED[name][3], ' '.join('%.0e' % v for v in prof)))
        assert dist >= OBSERVED[name][3] / 8 and dist >= 10 * quiet, (name, dist, quiet)
        assert prof[0] > prof[-1], (name, prof)


@pytest.mark.parametrize('S', [0, 3])
def test_f64_linear_gradient_oracle_is_the_chi2_gradient(S):
    """oracle_torch.grad_linear (the float64 reference of bhn_render_bwd: d sum(dimages images) / d params) with dimages =
    d chi^2 / d images is CpuTrainer.loss_and_grad's gradient to float64 rounding (the chain rule through the images), without and
    with Stokes planes; the emulator with its rounding off gives the same through its hand-written backward."""
    ks, bs, geom, hp, tf, tg = small_problem(4, 48, S, True)
    target, sigma, offset = tg
    scale = 0.7
    tr = ot.CpuTrainer(ks, bs, geom, hp)
    _, images, g0 = tr.loss_and_grad(tf, target, sigma, offset, scale, 'full')
    dimages = 2.0 * scale * (images - target - offset) / sigma ** 2
    assert dimages.shape == ((2, 3, 6, 5) if S else (2, 6, 5))
    g0 = ob.flat(g0)
    assert np.abs(g0).max() > 0
    g1 = ob.flat(ot.grad_linear(ks, bs, geom, hp, tf, dimages))
    assert rel(g1, g0) < 1e-13, rel(g1, g0)
    assert rel(ob.flat(tr.grad_linear(tf, dimages)), g0) < 1e-13
    for recipe in ('generic', 'fused128'):
        assert rel(ob.flat(ob.Bf16Trainer(ks, bs, geom, hp, recipe, rounding=False).grad_linear(tf, dimages)), g0) < 1e-12, recipe
    # another dimages (the frames swapped) gives another gradient: a frame offset cannot hide
    g2 = ob.flat(ot.grad_linear(ks, bs, geom, hp, tf, torch.flip(dimages, dims=(0,))))
    assert rel(g2, g0) > 1e-3
