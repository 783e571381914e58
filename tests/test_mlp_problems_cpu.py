"""CPU pins of what tests/mlp_problems.py builds: every random_problem of the GPU suite (the shapes of mlp_bounds.RANDOM_SHAPES and
GENERAL_SHAPES, two dropped-samples variants and a nudged one) and every small_problem of test_oracle_bf16_cpu, by sha256 of their
INPUTS as the builders in test_gpu_backward.py / test_oracle_bf16_cpu.py drew them before they moved here.  The float64 references are
not hashed: autograd output may depend on the BLAS thread count.  (The frame-chunk and buffer-contract problems, built on the same ray
grid, are pinned by tests/test_buffer_contract_cases_cpu.py.)"""
import hashlib

import numpy as np
import pytest

from mlp_bounds import GENERAL_SHAPES, RANDOM_SHAPES, STOKES4_SHAPES
from mlp_problems import random_problem_inputs, small_problem

# (width, depth, S, posenc degree): sha256, first 16 hex digits
RANDOM_PINS = {
    (256, 4, 0, 3): '1345e78b57d99fbe',
    (128, 4, 3, 3): '63ef3d09ea6d7196',
    (64, 8, 2, 3): 'c2cde755e9a76582',
    (32, 6, 0, 3): 'e36ea33681974980',
    (128, 4, 0, 0): '59047c34e07eabad',
    (256, 4, 3, 1): '6c6d9b6672f51947',
    (64, 4, 0, 2): '86566e9288df1c26',
    (128, 4, 2, 4): '5170348e8dc0cdb5',
    (100, 4, 0, 3): 'c3e8f93737d4307b',
    (48, 4, 3, 3): '7013ca7c89a01238',
    (200, 6, 0, 2): '3958909904b66770',
    (20, 4, 0, 3): '3892fcac7ef8424f',
    (64, 5, 0, 3): 'b568d8a2dd8a3394',
    (128, 7, 2, 3): '28ade17bc6c611d6',
    (32, 3, 0, 3): '5f87cc257db7d312',
    (64, 2, 3, 2): '5283e8993dd9665d',
    (256, 5, 0, 3): 'b61c382fa09124c4',
    (256, 8, 0, 3): 'd1deaed99fb528dc',
    (256, 8, 3, 3): '1b6caa6742a35a99',
    (64, 4, 1, 3): '9c21c36648ccff31',
    (256, 6, 1, 2): '0891b0c4f96c906d',
    (256, 2, 0, 3): '40c49acc2b0ab3de',
    (128, 4, 3, 5): '628ba32b47d5cb34',
    (512, 4, 0, 3): 'ab9bc098a66bfafe',
    (300, 3, 1, 6): 'fcb8016710ca1ead',
    (64, 2, 0, 7): '1ee72de2f84ce874',
    (384, 8, 2, 4): 'dc05eaa8bf54e2cf',
    (512, 8, 0, 8): 'b4637d3d6fdcdcc1',
    (40, 5, 3, 10): 'd4c6d83affe3353a',
}
# four Stokes planes (mlp_bounds.STOKES4_SHAPES): the V row is drawn behind I and chi, so the pins above did not move when it came
STOKES4_PINS = {
    (128, 4, 4, 3): 'e29278871998b27a',
    (256, 4, 4, 3): '9a4e0c18744d3474',
    (256, 8, 4, 3): 'a41ab502b08cd0bf',
    (64, 6, 4, 3): '19b91bf313a4d472',
    (32, 3, 4, 3): '751874b9adbeeaf4',
    (256, 2, 4, 3): 'a309f539718ae4d2',
    (288, 4, 4, 3): 'daab2b97ed5026ca',
    (512, 4, 4, 6): 'fef090c9a24001ce',
}
# the tie adjudications: the tied ray samples dropped (Doppler weight 0), every weight nudged by a relative 1e-4
VARIANT_PINS = {
    (128, 7, 2, 3, ('drop_ties', True)): '710888c883a5d2f0',
    (256, 8, 0, 3, ('drop_ties', True)): '4378cedf8a37823f',
    (64, 4, 0, 2, ('nudge', 0.0001)): 'efb902851b2cf56a',
}
# (depth, width, S, do_skip) of test_oracle_bf16_cpu's identity tests
SMALL_PINS = {
    (2, 48, 0, True): '5bebd12dc0a2e7af',
    (2, 48, 1, False): 'a9660fa6b23ec098',
    (3, 48, 3, True): 'ebd842f8297028d2',
    (3, 48, 0, False): 'a3f99bd1e73df0cf',
    (4, 48, 1, True): '1a402647b42603f0',
    (4, 48, 3, False): '8139ff5108efeb75',
    (8, 48, 0, True): '0cbdaace616d3c4f',
    (8, 48, 3, False): '9fd0e24e8a0a2ad7',
    (5, 48, 1, True): 'd943217043ea3d2f',
    (4, 48, 0, True): '383f0d996dc5deff',
    (4, 48, 3, True): '19e189fb44f55acb',
}


def checksum(arrays):
    h = hashlib.sha256()
    for k, v in arrays:
        a = np.ascontiguousarray(np.asarray(v.detach().numpy() if hasattr(v, 'detach') else v, dtype=np.float64))
        h.update(k.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    return h


def random_checksum(prob):
    """Every array of g, then target, sigma, offset, t_frames and t_inj."""
    return checksum([(k, prob['g'][k]) for k in sorted(prob['g'])]
                    + [(k, prob[k]) for k in ('target', 'sigma', 'offset', 't_frames', 't_inj')]).hexdigest()[:16]


def small_checksum(ks, bs, geom, hp, tf, tg):
    h = checksum([('k%d' % i, k) for i, k in enumerate(ks)] + [('b%d' % i, b) for i, b in enumerate(bs)]
                 + [(k, geom[k]) for k in sorted(geom) if geom[k] is not None] + [('t_frames', tf)] + [('tg%d' % i, v) for i, v in enumerate(tg)])
    h.update(repr(sorted((k, float(v)) for k, v in hp.items())).encode())
    return h.hexdigest()[:16]


def test_pins_cover_the_suite():
    assert list(RANDOM_PINS) == RANDOM_SHAPES + GENERAL_SHAPES
    assert list(STOKES4_PINS) == STOKES4_SHAPES and all(s[2] == 4 for s in STOKES4_SHAPES)


@pytest.mark.parametrize('shape', list(RANDOM_PINS) + list(STOKES4_PINS), ids=lambda s: '%dx%d-S%d-deg%d' % (s[1], s[0], s[2], s[3]))
def test_random_problem_is_drawn_bit_for_bit(shape):
    prob = random_problem_inputs(*shape)
    assert prob['g']['J'].shape[:1] == (shape[2],) if shape[2] else not prob['g']['J'].ndim
    assert random_checksum(prob) == {**RANDOM_PINS, **STOKES4_PINS}[shape]


def test_tie_adjudication_variants_are_drawn_bit_for_bit():
    for (w, d, S, deg, (key, value)), want in VARIANT_PINS.items():
        assert random_checksum(random_problem_inputs(w, d, S, deg, **{key: value})) == want, (w, d, S, deg, key)


def test_small_problem_is_drawn_bit_for_bit():
    for (depth, width, S, do_skip), want in SMALL_PINS.items():
        assert small_checksum(*small_problem(depth, width, S, do_skip)) == want, (depth, width, S, do_skip)
