"""Every training path but the bf16 width-256 one keeps its bits, and the pinned bits are the right bits.

test_step_keeps_its_bits: two gradient steps (pack -> training forward -> chi^2 -> backward -> Adam) of every case of
tests/step_cases.py -- the fused 4x128 backward (bwd128_kernel + reduce128_kernel), the W_out fold at widths 64 and 128, the generic
tape backward, the 8-bit tape, the fused f32 kernels and the general path in both modes -- give the loss vector, the images, the flat
gradient, the parameters and Adam's m and v that tests/golden/step_same_bits.json recorded: a SHA-256 and a strided sample of at most
64 elements per array (21 cases: the file stays small; the SHA-256 is what decides, the sample only says where the first difference
lies), in the format of tests/golden/w256_same_bits.json (test_gpu_w256_same_bits, the guard of the bf16 width-256 path;
tests/same_bits.py is what the two share).  A change to a step kernel that claims "same arithmetic" passes this file unchanged;
one that moves a rounding, an operand order, the tape layout or the job split does not, and has to say so and re-record the path it
changed (python tests/test_gpu_step_same_bits.py --record: every case runs twice in one process, and only a case whose two runs agree
bit for bit is written; the others are reported with the array and the first differing index).  Every case asserts the path it
reaches (gpu_support.assert_path) and its layout, so a case that no longer runs the kernels it is listed for fails instead of pinning
other ones, and holds engine.render's images equal to engine.render_train's bit for bit.

The slab counts of the weight-gradient kernels and the grouping of their sums follow the number of compute units, so the recorded bits
are those of a 256-CU device (MI355X); on any other device the bit tests skip.

test_first_step_against_its_reference: what the FIRST step of every case -- and of the seven cases of test_gpu_w256_same_bits -- gives
on the parameters before it (loss, images, gradient) against the reference of the case (step_cases.reference): the float64 oracle for
the f32 mode (images 1e-5, gradient GTOL / L2TOL['f32'], ReLU ties adjudicated), the bf16 emulator of the path for the bf16 mode
(mlp_bounds' caps: images 5e-4, gradient L2 3e-3, worst tensor 6e-3), and for the 8-bit tape the emulator for the images and the float64
oracle for the gradient by the bf16 mode's bounds (test_gpu_backward.test_tape8_mode_gradient's).  No bound here is new, and none
comes from the kernels under test.  One device run per case serves both tests."""
import json
import os
import sys
import time

import pytest
import torch

import step_cases as sc
import test_gpu_w256_same_bits as w256
from conftest import GOLDEN
from gpu_support import dev  # noqa: F401
from mlp_bounds import held_or_adjudicated
from same_bits import ARRAYS, CUS, first_difference, mismatches, record_of, run_case

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'step_same_bits.json')
SAMPLE = 64                                # elements of the strided sample of an array in FIXTURE (w256_same_bits.json: 1,024)
LIMIT = 1 << 20                            # bytes: no committed file is larger
CASES = sc.CASES
W256 = ['w256_' + n for n in w256.CASES]

_RUNS = {}


def step_of(dev, name, drop=None, steps=2):
    """(bits, first step) of a case of either table; the whole two-step run of a case is made once and shared by the tests."""
    if drop is None and name in _RUNS:
        return _RUNS[name]
    first, t0 = {}, time.time()
    if name in CASES:
        out = run_case(dev, name, CASES[name], sc.check_path, first, drop, steps)
    else:
        out = w256.run_case(dev, name[len('w256_'):], first, drop, steps)
    first['seconds'] = time.time() - t0
    if drop is None:
        _RUNS[name] = (out, first)
    return out, first


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
    out, first = step_of(dev, name)
    print('\n[same bits] %-22s %-11s flags %s  two steps %.2f s' % (name, CASES[name]['path'], first['flags'], first['seconds']))
    bad = mismatches(out, recorded['cases'][name], ARRAYS)
    assert not bad, '%s: %s' % (name, ' | '.join(bad))


@pytest.mark.parametrize('name', list(CASES) + W256)
def test_first_step_against_its_reference(dev, name):
    c = CASES[name] if name in CASES else w256.CASES[name[len('w256_'):]]
    recipe = sc.recipe_of(c)
    b = sc.bounds(c, recipe)

    def figures(drop):
        t0 = time.time()
        ref = sc.reference(name, c, recipe, drop)
        t1 = time.time()
        r = sc.errors(step_of(dev, name, drop, steps=1 if drop is not None else 2)[1], ref)
        print('\n[first step] %-22s %-11s vs %-8s %s   (reference %.1f s)' % (
            name, recipe, sc.reference_kind(c), '  '.join('%s %.2e' % kv for kv in r.items()), t1 - t0))
        return r

    ok, second = held_or_adjudicated(name, figures(None), lambda r: all(r[k] < b[k] for k in b),
                                     lambda: sc.reference_ties(name, c, recipe), figures)
    assert ok, (name, recipe, 'bounds', b, 'NOT a tie: without the tied samples' if second is not None else 'no tied samples', second)


def record(path):
    """Every case twice on this device; a case whose two runs agree bit for bit is written, the others are reported."""
    device = torch.device('cuda:0')
    assert torch.cuda.get_device_properties(device).multi_processor_count == CUS
    cases, unpinned = {}, {}
    for n in CASES:
        first, t0 = {}, time.time()
        a = run_case(device, n, CASES[n], sc.check_path, first)
        t1 = time.time()
        b = run_case(device, n, CASES[n], sc.check_path)
        d = first_difference(a, b)
        print('%-22s %-11s flags %s  two steps %.2f s / %.2f s  %s' % (n, CASES[n]['path'], first['flags'], t1 - t0, time.time() - t1,
                                                                     'reproducible' if d is None else 'NOT REPRODUCIBLE: %s' % (d,)), flush=True)
        if d is None:
            cases[n] = {k: record_of(v, SAMPLE) for k, v in a.items()}
        else:
            unpinned[n] = d
    doc = dict(compute_units=CUS, cases=cases)
    with open(path, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    size = os.path.getsize(path)
    print('recorded %d of %d cases -> %s (%d bytes)' % (len(cases), len(CASES), path, size))
    for n, d in unpinned.items():
        print('not pinned: %s: array %s, first differing index %d (%08x / %08x)' % ((n,) + d))
    assert size <= LIMIT, 'the fixture is larger than a committed file may be: lower SAMPLE (the SHA-256 stays authoritative)'


if __name__ == '__main__':
    if sys.argv[1:2] != ['--record'] or len(sys.argv) > 3:
        sys.exit('usage: python tests/test_gpu_step_same_bits.py --record [FILE]   (on a %d-CU device: rewrites %s, or FILE)' % (CUS, FIXTURE))
    record(sys.argv[2] if len(sys.argv) == 3 else FIXTURE)
