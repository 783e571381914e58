"""CPU checks of the same-bits guards (test_gpu_w256_same_bits, test_gpu_step_same_bits): every case of both tables builds, draws
the inputs that were recorded (sha256 pins: a changed draw cannot silently change what a fixture holds) and is listed for the path the
library's selection rules give it and for the layout its ray set has; both fixtures parse, hold a record of every array of every case
and of the length the case's shapes imply; and same_bits' comparison tells an equal array from one with a flipped bit, naming the
element.  Nothing here needs a device."""
import hashlib
import json
import os

import numpy as np
import pytest

import same_bits as sb
import step_cases as sc
import test_gpu_w256_same_bits as w256
from conftest import GOLDEN, mask_tie_points
from gpu_support import assert_path, expected_flags
from oracle import oracle_bf16 as ob
from test_mlp_harness_cpu import Eng, Geom

TABLES = {'step': (sc.CASES, os.path.join(GOLDEN, 'step_same_bits.json')), 'w256': (w256.CASES, os.path.join(GOLDEN, 'w256_same_bits.json'))}
ALL = [(t, n) for t, (cases, _) in TABLES.items() for n in cases]
# sha256 (first 16 hex digits) of the inputs of every case: the arrays of g, the frame times and the chi^2 targets
PINS = {
    ('step', 'f128_full'): '6fc96168a67a592f',
    ('step', 'f128_w113_noskip'): '81843f09e47abae7',
    ('step', 'f128_w97_s3_lc'): 'fb270319fd5c7d2b',
    ('step', 'f128_rows48'): '0cd6569300614ab4',
    ('step', 'f128_rows47'): '1271ba1960424d5d',
    ('step', 'f128_compact'): '6f4c1b71e4a21c84',
    ('step', 'f128_frame_groups'): '49ff4ec5bd7498e0',
    ('step', 'fold_4x64'): '2849aa45325fca93',
    ('step', 'fold_5x128'): '8ea9a9f5f40f6766',
    ('step', 'generic_2x32'): '922dd1c59ae6ee64',
    ('step', 't8_4x256'): '29d1a42035d15da3',
    ('step', 't8_8x256_s4'): 'be18c7838133fe43',
    ('step', 'f32_4x32'): '0586cc2b47239deb',
    ('step', 'f32_4x128'): '6fc96168a67a592f',
    ('step', 'f32_4x256'): '29d1a42035d15da3',
    ('step', 'f32_4x128_s3_lc'): '3d8c2c4b2a52c4c2',
    ('step', 'f32_4x256_compact'): 'faa8eaca6e4b8bd7',
    ('step', 'gen_4x160_deg5_f32'): 'f5f86d6aa2adcf3b',
    ('step', 'gen_4x160_deg5_bf16'): 'f5f86d6aa2adcf3b',
    ('step', 'gen_4x257_deg5_f32'): '6d58f6955b83d765',
    ('step', 'gen_4x257_deg5_bf16'): '6d58f6955b83d765',
    ('w256', 'full_tiles'): '09f5f759885735fd',
    ('w256', 'ragged_tile'): '0574cbdd234595c0',
    ('w256', 'stokes3_lc'): '0c5df2b6b0aeff2d',
    ('w256', 'compact'): 'faa8eaca6e4b8bd7',
    ('w256', 'depth3'): 'ff8ec1b1aa9f0abd',
    ('w256', 'depth5'): '5c668851347b32ca',
    ('w256', 'frame_groups'): '0574cbdd234595c0',
}


def checksum(c):
    prob = sb.case_problem(c)
    h = hashlib.sha256()
    for k, v in ([(k, prob['g'][k]) for k in sorted(prob['g'])] + [('t_inj', prob['t_inj'])]
                 + list(zip(('target', 'sigma', 'offset'), sb.case_targets(c, prob)))):
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        h.update(k.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()[:16], prob


@pytest.fixture(scope='module')
def fixtures():
    out = {}
    for t, (_, path) in TABLES.items():
        with open(path) as f:
            out[t] = json.load(f)
    return out


def test_pins_cover_both_tables():
    assert sorted(PINS) == sorted(ALL)
    assert all(c['why'] and c['path'] in ('fused128', 'fold', 'generic', 't8', 'f32', 'general', 'general f32') for c in sc.CASES.values())
    # every unguarded path the table is there for has a case
    assert {c['path'] for c in sc.CASES.values()} == {'fused128', 'fold', 'generic', 't8', 'f32', 'general', 'general f32'}
    assert 'ga0_chain' not in {sc.recipe_of(c) for c in sc.CASES.values()} and {sc.recipe_of(c) for c in w256.CASES.values()} == {'ga0_chain'}


@pytest.mark.parametrize('table,name', ALL, ids=['%s-%s' % a for a in ALL])
def test_case_builds_as_recorded_and_is_listed_for_its_path(table, name):
    c = TABLES[table][0][name]
    digest, prob = checksum(c)
    assert digest == PINS[(table, name)]
    H, Wd, G, B = c['shape']
    g = prob['g']
    assert g['coords'].shape == (3, H, Wd, G) and len(g['t_frames']) == B and (g['J'].shape[0] if c['S'] else g['J'].ndim) == c['S']
    assert not mask_tie_points(g).any()                   # no domain or injection mask decided within f32 rounding
    assert c['cap'] is None or 0 < c['cap'] < B
    groups, compact = sc.layout_of(c, prob)
    if table == 'w256':
        assert (groups, compact) == w256.LAYOUT[name]
        return
    # the layout and the path the case is listed for are the ones its ray set and the selection rules give
    assert (groups, compact) == (c['groups'], c['compact'])
    recipe, general = sc.recipe_of(c), sc.is_general(c)
    assert recipe == c['path'] and general == c['path'].startswith('general')
    want = expected_flags(recipe)
    if c['mode'] != 'f32':
        assert ob.recipe_for(want) == sc.emulator_recipe(c, recipe) and ob.RECIPES[sc.emulator_recipe(c, recipe)]
    else:
        assert not (want['fused128'] or want['ga0_chain'] or want['drop_ga'])
    # ... and check_path's judgement accepts exactly those flags (gpu_support.assert_path on a stand-in engine)
    tg = c['tile_groups'] or 8
    assert_path(name, Eng(recipe, tile_groups=tg), Geom(compact, 32 * groups), c['mode'], c['path'], general, compact=c['compact'], tile_groups=c['tile_groups'])
    other = 'fold' if recipe not in ('fold', 't8') else 'fused128'          # (the 8-bit tape shows the fold's flags)
    if c['mode'] != 'f32':
        with pytest.raises(AssertionError):
            assert_path(name, Eng(other, tile_groups=tg), Geom(compact, 32 * groups), c['mode'], c['path'], general)
    if general:
        assert sc.general_ng(c) == sc.GENERAL_NG[name]
    if c['tile_groups']:
        assert (c['tile_groups'] == 12) == (groups >= 3072)                # the threshold of the fused 4x128 forward pair


def test_general_cases_sit_on_both_sides_of_the_ng_rule():
    assert sorted(sc.GENERAL_NG) == sorted(n for n, c in sc.CASES.items() if sc.is_general(c))
    assert set(sc.GENERAL_NG.values()) == {2, 4}


@pytest.mark.parametrize('table,name', ALL, ids=['%s-%s' % a for a in ALL])
def test_fixture_holds_every_array_of_the_case(fixtures, table, name):
    doc, c = fixtures[table], TABLES[table][0][name]
    assert doc['compute_units'] == sb.CUS and sorted(doc['cases']) == sorted(TABLES[table][0])
    rec, sizes = doc['cases'][name], sc.array_sizes(c)
    assert sorted(rec) == sorted(sb.ARRAYS) == sorted(sizes)
    for k in sb.ARRAYS:
        r = rec[k]
        assert r['n'] == sizes[k], (k, r['n'], sizes[k])
        assert r['stride'] >= 1 and len(r['sample']) == 8 * min(1024, -(-r['n'] // r['stride'])), k
        assert len(r['sha256']) == 64 and int(r['sha256'], 16) >= 0
        s = sb.sample_bits(r)
        assert s.dtype == np.uint32 and s.size == len(r['sample']) // 8
        assert np.isfinite(s.view(np.float32)).all(), k
    # Adam's second moment is a sum of squares; a training step leaves non-zero images and gradients
    assert (sb.sample_bits(rec['adam_v']).view(np.float32) >= 0).all()
    assert all(sb.sample_bits(rec[k]).any() for k in ('loss', 'images', 'grad', 'params', 'adam_m', 'adam_v'))


def test_array_sizes_are_the_networks():
    for t, n in ALL:
        c = TABLES[t][0][n]
        g = sb.case_problem(c)['g']
        assert sc.array_sizes(c)['grad'] == sum(g['kernel%d' % i].size + g['bias%d' % i].size for i in range(c['depth'] + 1)), (t, n)


@pytest.mark.parametrize('n', [1, 7, 1024, 1025, 55169])
def test_record_tells_an_equal_array_from_a_flipped_bit(n):
    rng = np.random.default_rng(n)
    u = sb.bits(rng.standard_normal(n).astype(np.float32))
    rec = sb.record_of(u)
    assert rec['n'] == n and rec['stride'] == max(1, -(-n // 1024)) and len(rec['sample']) == 8 * min(1024, -(-n // rec['stride']))
    assert np.array_equal(sb.sample_bits(rec), u[::rec['stride']][:1024])
    assert sb.mismatch('grad', u.copy(), rec) is None and sb.mismatches(dict(grad=u), dict(grad=rec), ('grad',)) == []
    # one bit of a sampled element: the message names its index and both words
    i = rec['stride'] * ((n // rec['stride']) // 2)
    v = u.copy(); v[i] ^= np.uint32(1)
    msg = sb.mismatch('grad', v, rec)
    assert msg is not None and 'first differing sampled element: index %d, %08x' % (i, v[i]) in msg and 'the recorded %08x' % u[i] in msg
    assert '1 of %d sampled differ' % (len(rec['sample']) // 8) in msg
    # one bit between the samples: the SHA-256 sees it, the message says that no sampled element differs
    if rec['stride'] > 1:
        v = u.copy(); v[i + 1] ^= np.uint32(1 << 31)
        msg = sb.mismatch('grad', v, rec)
        assert msg is not None and 'every sampled element (stride %d) is equal' % rec['stride'] in msg
    # another length
    msg = sb.mismatch('grad', u[:-1] if n > 1 else np.concatenate([u, u]), rec)
    assert msg is not None and 'recorded %d' % n in msg and 'sampled' not in msg
    # a lower sample length (a fixture that would otherwise be too large) is compared by its own stride
    small = sb.record_of(u, 16)
    assert len(small['sample']) <= 8 * 16 and sb.mismatch('grad', u, small) is None
    v = u.copy(); v[0] ^= np.uint32(2)
    assert 'index 0,' in sb.mismatch('grad', v, small)


def test_first_difference_names_the_array_and_the_index():
    a = {k: np.arange(10, dtype=np.uint32) for k in sb.ARRAYS}
    assert sb.first_difference(a, {k: v.copy() for k, v in a.items()}) is None
    b = {k: v.copy() for k, v in a.items()}
    b['params'][7] ^= np.uint32(4); b['adam_v'][2] ^= np.uint32(1)
    assert sb.first_difference(a, b) == ('params', 7, 7, 3)
