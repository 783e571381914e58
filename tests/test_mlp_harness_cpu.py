"""CPU checks that the judgement the MLP case tests share fails when it should: gpu_support.assert_path on hand-made tape_info flags,
mlp_bounds.held_or_adjudicated on hand-made figures, mlp_reference.tie_points on a stand-in emulator and the one reference cache."""
import types

import numpy as np
import pytest

import mlp_reference as mr
from gpu_support import assert_path, expected_flags
from mlp_bounds import first_difference, held_or_adjudicated, tensor_l2, tensor_label


class Eng:
    """engine.tape_info of a path: the flags of `recipe`, changed by `flags`."""

    def __init__(self, recipe, tile_groups=8, **flags):
        self.info = dict(flags=dict(expected_flags(recipe), **flags), fwd_groups_per_tile=tile_groups)

    def tape_info(self, groups):
        self.groups = groups
        return self.info


class Geom:
    def __init__(self, compact=False, P_eff=58 * 32):
        self.P_eff, self.compact = P_eff, (dict(n=1) if compact else None)


def test_assert_path_accepts_every_path_as_listed():
    for mode, recipe in (('bf16', 'generic'), ('bf16', 'fold'), ('bf16', 'ga0_chain'), ('bf16', 'fused128'), ('bf16', 'general'),
                         ('bf16_t8', 't8'), ('f32', 'f32'), ('f32', 'general f32'), ('f32', None)):
        eng = Eng(recipe or 'f32', tile_groups=12)
        flags, info = assert_path('case', eng, Geom(True, 33), mode, recipe, (recipe or '').startswith('general'), compact=True, tile_groups=12)
        assert flags is eng.info['flags'] and info is eng.info and eng.groups == 2
    assert_path('case', Eng('general', drop_ga=True), Geom(), 'bf16', 'general', True)         # drop_ga is not looked at on the general path


RAISES = [
    ('fold flags given as ga0_chain', Eng('fold'), 'bf16', 'ga0_chain', False, {}),
    ('fused128 flags given as fold', Eng('fused128'), 'bf16', 'fold', False, {}),
    ('fused128 flags given as generic', Eng('fused128'), 'bf16', 'generic', False, {}),
    ('ga0_chain without drop_ga', Eng('ga0_chain', drop_ga=False), 'bf16', 'ga0_chain', False, {}),
    ('t8 without drop_ga', Eng('generic'), 'bf16_t8', 't8', False, {}),
    ('t8 on the ga0_chain path', Eng('ga0_chain'), 'bf16_t8', 't8', False, {}),
    ('general flipped on', Eng('fold', general=True), 'bf16', 'fold', False, {}),
    ('general flipped off', Eng('general', general=False), 'bf16', 'general', True, {}),
    ('a fused recipe listed as general', Eng('general'), 'bf16', 'fold', True, {}),
    ('f32 general flipped', Eng('general f32'), 'f32', 'f32', False, {}),
    ('f32 with drop_ga', Eng('f32', drop_ga=True), 'f32', 'f32', False, {}),
    ('f32 with fused128', Eng('f32', fused128=True), 'f32', None, False, {}),
    ('compact expected', Eng('fold'), 'bf16', 'fold', False, dict(compact=True)),
    ('compact not expected', Eng('f32'), 'f32', 'f32', False, dict(compact=False, geom=Geom(True))),
    ('tile_groups', Eng('fused128', tile_groups=8), 'bf16', 'fused128', False, dict(tile_groups=12)),
]


@pytest.mark.parametrize('why,eng,mode,recipe,general,kw', RAISES, ids=[r[0] for r in RAISES])
def test_assert_path_raises(why, eng, mode, recipe, general, kw):
    kw = dict(kw)
    geom = kw.pop('geom', Geom())
    with pytest.raises(AssertionError):
        assert_path(why, eng, geom, mode, recipe, general, **kw)


class Calls:
    """ties / rerun stand-ins that count their calls."""

    def __init__(self, mask, second):
        self.mask, self.second, self.n_ties, self.n_rerun = np.asarray(mask), second, 0, 0

    def ties(self):
        self.n_ties += 1
        return self.mask

    def rerun(self, mask):
        assert mask is self.mask
        self.n_rerun += 1
        return self.second


WITHIN = lambda f: f['err'] < 1.0


def test_held_figures_are_not_adjudicated():
    c = Calls([True], dict(err=0.0))
    assert held_or_adjudicated('case', dict(err=0.5), WITHIN, c.ties, c.rerun, also=lambda s: False) == (True, None)
    assert (c.n_ties, c.n_rerun) == (0, 0)


def test_a_miss_is_excused_only_by_ties_whose_removal_meets_bounds_and_side_conditions(capsys):
    miss = dict(err=2.0)
    c = Calls([False, False], dict(err=0.0))                 # no tied sample: nothing to take out
    assert held_or_adjudicated('case', miss, WITHIN, c.ties, c.rerun) == (False, None) and (c.n_ties, c.n_rerun) == (1, 0)
    c = Calls([False, True], dict(err=1.5))                  # the rerun still misses
    assert held_or_adjudicated('case', miss, WITHIN, c.ties, c.rerun) == (False, c.second) and (c.n_ties, c.n_rerun) == (1, 1)
    c = Calls([False, True], dict(err=0.5, repro=False))     # inside the bounds, but the site's side condition fails
    assert held_or_adjudicated('case', miss, WITHIN, c.ties, c.rerun, also=lambda s: s['repro']) == (False, c.second) and (c.n_ties, c.n_rerun) == (1, 1)
    assert capsys.readouterr().out.count('NOT a tie') == 2
    c = Calls([True, True, False], dict(err=0.5, repro=True))
    assert held_or_adjudicated('the case', miss, WITHIN, c.ties, c.rerun, also=lambda s: s['repro']) == (True, c.second) and (c.n_ties, c.n_rerun) == (1, 1)
    assert capsys.readouterr().out == 'relu ties (the case): 2 tied ray samples taken out: adjudicated\n'


def Emulator(mask):
    """A stand-in for an emulator whose forward has the tied points `mask`."""
    return types.SimpleNamespace(relu_tie_points=lambda tf: mask.copy())


def test_tie_points_clears_samples_without_doppler_weight():
    g = dict(g=np.array([[[1.0, 0.0, 0.7], [0.0, 1.2, 0.9]]]))
    mask = np.array([[[True, True, False], [True, True, True]]])
    assert np.array_equal(mr.tie_points(g, Emulator(mask), None), mask & (g['g'] != 0))
    assert mr.tie_points(g, Emulator(mask), None).sum() == 3


def test_tie_points_of_the_float64_oracle_without_skips_goes_through_the_unrounded_emulator(monkeypatch):
    made = []

    def Trainer(ks, bs, geom, hp, recipe='generic', rounding=True):
        made.append((hp, rounding))
        return Emulator(np.ones((1, 2, 3), dtype=bool))

    def walks_the_skip_network(g, **kw):
        raise AssertionError('relu_tie_count on a network without skips')
    g = dict(g=np.ones((1, 2, 3)))
    monkeypatch.setattr(mr, 'oracle_inputs', lambda g: ('ks', 'bs', 'geom', dict(net_depth=4)))
    monkeypatch.setattr(mr.ob, 'Bf16Trainer', Trainer)
    monkeypatch.setattr(mr, 'relu_tie_count', walks_the_skip_network)
    assert mr.tie_points(g, None, None, do_skip=False).all()
    assert made == [(dict(net_depth=4, do_skip=False), False)]
    with pytest.raises(AssertionError):                     # with skips it is relu_tie_count's
        mr.tie_points(g, None, None)
    monkeypatch.setattr(mr, 'relu_tie_count', lambda g, return_points: (5, np.array([[[True, False, True], [False, False, False]]])))
    assert mr.tie_points(g, None, None).sum() == 2 and len(made) == 1


def test_cache_makes_once_keeps_dropped_apart_and_freezes():
    made = []

    def make():
        made.append(1)
        return dict(grad=np.zeros(3), images=np.ones((2, 2)), note='text')
    a = mr.cached('harness test', 'case', 'linear', 'fold', None, False, make)
    assert mr.cached('harness test', 'case', 'linear', 'fold', None, False, make) is a and len(made) == 1
    b = mr.cached('harness test', 'case', 'linear', 'fold', np.ones(2, dtype=bool), False, make)
    assert b is not a and mr.cached('harness test', 'case', 'linear', 'fold', np.zeros(2, dtype=bool), False, make) is b
    others = [mr.cached(*key, make) for key in (('other family', 'case', 'linear', 'fold', None, False), ('harness test', 'case 2', 'linear', 'fold', None, False),
                                               ('harness test', 'case', 'ties', 'fold', None, False), ('harness test', 'case', 'linear', None, None, False),
                                               ('harness test', 'case', 'linear', 'fold', None, True))]
    assert len({id(v) for v in others + [a, b]}) == 7 and len(made) == 7
    for ref in (a, b):
        with pytest.raises(ValueError):
            ref['grad'][0] = 1.0
        with pytest.raises(ValueError):
            ref['images'][0, 0] = 0.0
    mask = mr.cached('harness test', 'case', 'mask', None, None, False, lambda: np.zeros(4, dtype=bool))
    with pytest.raises(ValueError):
        mask[0] = True


def test_dropped_zeroes_the_doppler_weight_of_the_samples_and_nothing_else():
    prob = dict(g=dict(g=np.array([0.5, 0.7, 0.9]), dtau=np.ones(3)), B=3)
    assert mr.dropped(prob, None) is prob
    out = mr.dropped(prob, np.array([False, True, False]))
    assert out['g']['g'].tolist() == [0.5, 0.0, 0.9] and out['g']['dtau'] is prob['g']['dtau'] and out['B'] == 3
    assert prob['g']['g'].tolist() == [0.5, 0.7, 0.9]


def test_small_pieces():
    ref = np.array([1.0, 2.0, 0.0, 0.0, 4.0])
    got = np.array([1.0, 2.2, 0.0, 0.0, 3.0])
    cuts = [0, 2, 4, 5]
    assert tensor_l2(got, ref, cuts, True) == [pytest.approx(0.2 / np.sqrt(5.0)), 0.0, 0.25]
    with np.errstate(invalid='ignore'):
        assert np.isnan(tensor_l2(got, ref, cuts, False)[1])
    assert [tensor_label(i) for i in range(4)] == ['K0', 'b0', 'K1', 'b1']
    a = np.array([1.0, -0.0, np.nan], dtype=np.float32)
    assert first_difference(a, a.copy()) is None                                  # bitwise: NaN equals itself ...
    assert first_difference(a, np.array([1.0, 0.0, np.nan], dtype=np.float32)) == (1, -0.0, 0.0)       # ... and -0 is not +0
