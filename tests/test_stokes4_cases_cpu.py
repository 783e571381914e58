"""CPU proof that the comparators of test_gpu_stokes4 see a slip in the fourth Stokes plane, case by case: every mutant of
stokes4_cases.MUTANTS, built into the reference the device is compared with (the float64 oracle for an f32 case, the bf16 emulator of
the case's recipe for a bf16 one), lands at least 5x outside the bound of at least one figure the GPU test asserts -- and the faithful
bf16 emulator, standing in for the bf16 kernels, lands inside the float64 bounds that test holds them to.  Also: the problem builder
draws a fourth row, refuses a fifth, and the S = 4 problems are pinned by sha256 next to the others (test_mlp_problems_cpu)."""
import numpy as np
import pytest

import stokes4_cases as sc
from mlp_bounds import STOKES4_SHAPES
from mlp_problems import stokes_factors

PARAMS = [(name, mode) for name, c in sc.CASES.items() for mode in c['modes']]


def test_stokes_factors_draws_the_fourth_row_and_refuses_a_fifth():
    shape = (3, 5, 7)
    J = stokes_factors(np.random.default_rng(1), shape, 4)
    assert J.shape == (4,) + shape
    I, Q, U, V = J
    assert (np.abs(V) <= 0.5 * I).all() and np.abs(V).max() > 0.25 * I.min() and (Q ** 2 + U ** 2 + V ** 2 <= I ** 2).all()
    # the rows of S <= 3 do not know about V: the same generator state gives the same I, Q, U, and the draws behind them stay in place
    for S in (1, 2, 3):
        rng = np.random.default_rng(1)
        assert np.array_equal(stokes_factors(rng, shape, S), J[:S])
        rng3 = np.random.default_rng(1)
        stokes_factors(rng3, shape, 3)
        assert rng.uniform() == rng3.uniform()
    for S in (0, 5, -1):
        with pytest.raises(ValueError):
            stokes_factors(np.random.default_rng(1), shape, S)


def test_case_table():
    assert [(c['width'], c['depth'], sc.S, c['deg']) for c in sc.CASES.values() if c['kind'] == 'chi2' and c['dt'] == 'full'] == STOKES4_SHAPES
    assert set(sc.SHAPE_WHY) == set(STOKES4_SHAPES)
    assert all(c['why'] for c in sc.CASES.values())
    # every bf16 case has its measured figures on record: its bounds are 4x those, not only the caps
    from mlp_bounds import OBSERVED
    assert all(len(OBSERVED[name]) == 5 for name, c in sc.CASES.items() if 'bf16' in c['modes'])
    # the paths the cases are listed for
    recipes = {name: sc.case_recipe(name, 'bf16') for name, c in sc.CASES.items() if 'bf16' in c['modes']}
    assert recipes['4x128 S4 deg3'] == 'fused128' and recipes['4x256 S4 deg3'] == recipes['8x256 S4 deg3'] == 'ga0_chain'
    assert recipes['6x64 S4 deg3'] == recipes['3x32 S4 deg3'] == 'fold' and recipes['2x256 S4 deg3'] == 'generic'
    assert recipes['4x288 S4 deg3'] == recipes['4x512 S4 deg6'] == recipes['4x288 S4 ragged'] == 'general'
    # the combine through LDS runs on the 4-, 8- and 12-wave kernels and on the general path
    combine = {(c['width'], m) for c in sc.CASES.values() if not c['direct'] for m in c['modes']}
    assert {(256, 'f32'), (256, 'bf16'), (64, 'f32'), (64, 'bf16'), (288, 'f32'), (288, 'bf16'), (128, 'bf16')} <= combine


def test_stride3_reads_plane_s_of_frame_b_at_3b_plus_s():
    import torch
    x = torch.arange(3 * 4 * 2, dtype=torch.float64).reshape(3, 4, 2)
    y = sc.stride3(x)
    flat = x.reshape(12, 2)
    for b in range(3):
        for s in range(4):
            assert torch.equal(y[b, s], flat[3 * b + s])
    assert torch.equal(y[0, :3], x[0, :3]) and not torch.equal(y[1], x[1])


@pytest.mark.parametrize('name,mode', PARAMS)
def test_bounds_see_every_mutant(name, mode):
    r = sc.case_references(name, mode)
    prob, ref64, ref_abs, emu, cuts = r['prob'], r['ref64'], r['ref_abs'], r['emu'], r['cuts']
    b = sc.bounds(name, mode)
    g = prob['g']
    assert g['J'].shape[0] == 4 and ref64['images'].shape[1] == 4
    # plane V is a fraction of plane I, which is why it gets a figure of its own
    peak = np.abs(ref64['images']).reshape(-1, 4, ref64['images'].shape[-1]).max(axis=(0, 2))
    assert 0.02 * peak[0] < peak[3] < 0.3 * peak[0], peak
    # which cases take the direct adds and which the combine through LDS (fused_fwd.hip fused_fill_args: ray_direct)
    c, G = sc.CASES[name], g['coords'].shape[-1]
    if c['compact']:
        from bhnerf_amd import engine
        assert 0 < len(r['r64'].idx) < 0.9 * g['coords'][0].size              # (engine.COMPACT_BELOW)
        assert (engine.ray_span(r['r64'].ray) in (1, 2)) == c['direct']
    else:
        assert len(r['r64'].idx) == g['coords'][0].size
        assert (G <= 33 or (G <= 64 and G % 32 == 0)) == c['direct']
    if mode == 'bf16':
        f = sc.figures(emu, ref64, ref_abs, cuts)
        print('\n[stokes4 cpu] %-24s emulator (%s) vs f64 oracle: %s' % (name, sc.case_recipe(name, mode), sc.describe(f)))
        assert sc.within(f, {k: v for k, v in b.items() if not k.startswith('em_')}), (name, f)
    faithful = ref64 if mode == 'f32' else emu
    ref = r['r64'] if mode == 'f32' else r['rem']
    for m in sc.MUTANTS:
        out = sc.outputs(name, ref, prob, m)
        # (the per-plane figure of a mutant of the emulator is taken against the oracle, as the GPU test takes the device's)
        f = sc.figures(out, ref64, ref_abs, cuts, None if mode == 'f32' else faithful)
        rt = sc.ratios(f, b)
        worst = max(rt, key=rt.get)
        print('[stokes4 cpu] %-24s %-5s %-24s %s   -> %.1fx its bound in %s' % (name, mode, m, sc.describe(f), rt[worst], worst))
        assert rt[worst] >= 5.0 or not sc.fits(name, m), (name, mode, m, rt)
