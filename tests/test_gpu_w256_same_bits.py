"""The bf16 width-256 training step keeps its bits: two gradient steps (pack -> training forward -> chi^2 -> delta chain -> dW ->
slab reduce -> Adam) of every case below give the loss vector, the images, the flat gradient, the parameters and Adam's m and v
that tests/golden/w256_same_bits.json recorded -- a SHA-256 and a strided sample of at most 1,024 elements per array, taken from the
build before the first instruction-count change to fused_common.h / fused_fwd.hip / fused_bwd.hip / bwd_common.h.  A change to those
kernels that claims "same arithmetic, fewer instructions" passes this file unchanged; one that moves a rounding, an operand order,
the tape layout or the job split does not, and has to say so and re-record (python tests/test_gpu_w256_same_bits.py --record).

Every case also holds engine.render's images equal to engine.render_train's bit for bit (the inference forward and the training
forward run the same ring step on the same packed weights).

The slab count of the weight-gradient kernel and the grouping of its sums follow the number of compute units, so the recorded bits
are those of a 256-CU device (MI355X); on any other device the test skips.

The other training paths (fused 4x128, the W_out fold at widths 32 ... 128, the generic tape backward, the 8-bit tape, f32, the general
path) are pinned the same way by tests/test_gpu_step_same_bits.py, which also holds the first step of the cases below to the bf16
emulator; tests/same_bits.py is what the two files share.

Cases (all 4 x 256-class networks in bf16, posenc degree 3, built by mlp_problems.random_problem_inputs):
    full_tiles     depth 4, 2 frames, 8 x 5 = 40 rays x 64 samples, all-active domain: 80 groups = 10 tiles of 8 per frame, fewer
                   tiles than workgroups, the last tile of each frame full
    ragged_tile    depth 4, 3 frames, 37 rays x 64 samples: 74 groups per frame, the last tile holds 2 groups of 8
    stokes3_lc     depth 4, 2 frames, 37 rays x 64 samples, three Stokes planes, light-curve loss 'lc'
    compact        depth 4, 3 frames, the ragged 9 x 7 x 50 grid in the shell domain: a point-compacted layout whose rays span at
                   most two 32-point groups
    depth3         depth 3 (the smallest depth with the ga0 chain), 2 frames, 37 rays x 64 samples
    depth5         depth 5 (odd depth: the output layer takes the skip input), 2 frames, 37 rays x 64 samples
    frame_groups   depth 4, 3 frames, 37 rays x 64 samples, workspace capped to a tape of 2 frames: groups of 2 + 1"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import same_bits
from conftest import GOLDEN
from gpu_support import dev  # noqa: F401
from mlp_problems import RANDOM_PROBLEM_DOMAIN, RANDOM_PROBLEM_SHAPE
from same_bits import ARRAYS, CUS, mismatches, record_of

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'w256_same_bits.json')
ALL_ACTIVE = (8.0, 0.0, np.inf, np.inf)
# name: depth, Stokes planes, (rays H, rays W, samples, frames), domain, loss, frames of tape the workspace is capped to (None: all)
CASES = {
    'full_tiles': dict(depth=4, S=0, shape=(8, 5, 64, 2), domain=ALL_ACTIVE, dt='full', cap=None),
    'ragged_tile': dict(depth=4, S=0, shape=(37, 1, 64, 3), domain=ALL_ACTIVE, dt='full', cap=None),
    'stokes3_lc': dict(depth=4, S=3, shape=(37, 1, 64, 2), domain=ALL_ACTIVE, dt='lc', cap=None),
    'compact': dict(depth=4, S=0, shape=RANDOM_PROBLEM_SHAPE, domain=RANDOM_PROBLEM_DOMAIN, dt='full', cap=None),
    'depth3': dict(depth=3, S=0, shape=(37, 1, 64, 2), domain=ALL_ACTIVE, dt='full', cap=None),
    'depth5': dict(depth=5, S=0, shape=(37, 1, 64, 2), domain=ALL_ACTIVE, dt='full', cap=None),
    'frame_groups': dict(depth=4, S=0, shape=(37, 1, 64, 3), domain=ALL_ACTIVE, dt='full', cap=2),
}
# what the layout of each case must be for the case to test what it is listed for: (groups per frame, point-compacted)
LAYOUT = {'full_tiles': (80, False), 'ragged_tile': (74, False), 'stokes3_lc': (74, False), 'compact': (21, True), 'depth3': (74, False),
          'depth5': (74, False), 'frame_groups': (74, False)}


def check_layout(name, eng, geom, groups, flags):
    assert (groups, geom.compact is not None) == LAYOUT[name], (name, groups, geom.compact is not None)
    if geom.compact is not None:
        assert geom.compact['ray_span'] <= 2, (name, geom.compact['ray_span'])
    assert not flags['general'] and not flags['fused128'] and flags['ga0_chain'] and flags['drop_ga'], (name, flags)


def run_case(dev, name, first=None, drop=None, steps=2):
    """Two gradient steps of the case `name` on a fresh predictor -> {array name: uint32 bits}; asserts the layout the case is listed
    for and render == render_train on the parameters the two steps left (same_bits.run_case)."""
    return same_bits.run_case(dev, name, CASES[name], check_layout, first, drop, steps)


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(CASES))
def test_step_keeps_its_bits(dev, recorded, name):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if cus != CUS:
        pytest.skip('the recorded bits are those of a %d-CU device (slab count and grouping of the sums); this one has %d' % (CUS, cus))
    assert recorded['compute_units'] == CUS and sorted(recorded['cases']) == sorted(CASES)
    out = run_case(dev, name)
    want = recorded['cases'][name]
    bad = mismatches(out, want, ARRAYS)
    assert not bad, '%s: %s' % (name, ' | '.join(bad))


if __name__ == '__main__':
    if sys.argv[1:2] != ['--record'] or len(sys.argv) > 3:
        sys.exit('usage: python tests/test_gpu_w256_same_bits.py --record [FILE]   (on a %d-CU device: rewrites %s, or FILE)' % (CUS, FIXTURE))
    FIXTURE = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
    device = torch.device('cuda:0')
    assert torch.cuda.get_device_properties(device).multi_processor_count == CUS
    doc = dict(compute_units=CUS, cases={n: {k: record_of(v) for k, v in run_case(device, n).items()} for n in CASES})
    with open(FIXTURE, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d cases -> %s (%d bytes)' % (len(CASES), FIXTURE, os.path.getsize(FIXTURE)))
