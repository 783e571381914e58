"""The weighted-term losses keep their bits: libbhnerf_eht.so, libbhnerf_cls.so, libbhnerf_pol.so and libbhnerf_reg.so through
engine.chi2_eht / chi2_volume give what tests/golden/eht_same_bits.json recorded -- a SHA-256 and a strided sample of at most 32
elements per array (some 200 arrays: half the step guard's 64 keeps the file well below that guard's), in the format of
tests/golden/step_same_bits.json (tests/same_bits.py is what the guards share).

The cases are the existing tables', nothing is generated here:
  uv   every (name, Sx) of eht_edge_cases.UV_PARAMS: observe() as float32 pairs and, per dtype of the case, the loss and dimages;
       the loss of the want_grad=False call is asserted to be the same float and recorded too;
  cls  every CLS_PARAMS entry at CLS_DTYPE and closure_cases.WEIGHTS, and 'amp' alone and 'cphase+logcamp' on 'w300':
       op.last_terms (4 floats) and dimages;
  pol  every POL_PARAMS entry at 'pvis+m', and 'pvis' alone and 'm' alone on 'w300' (Sx 3 and 4): op.last_terms (3 floats), dimages;
  vol  every case of vol_reg_cases.ALL_CASES through engine.chi2_volume on a VolumePrior of the case's spacing, weights and eps:
       last_terms, last_per_volume and dvolumes.

The plans of these kernels follow the sizes of a call only (no file of the four libraries reads the compute-unit count), so the
record carries no condition on the device.  A change that claims "same arithmetic" passes this file with the fixture unchanged; one
that moves a rounding or the order of a sum does not.  python tests/test_gpu_eht_same_bits.py --record [FILE] runs every case twice
in one process and writes the cases whose two runs agree bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN                                            # noqa: E402  (first: it puts the package on the path)
import closure_cases as K                                              # noqa: E402
import eht_edge_cases as T                                             # noqa: E402
import eht_uv_cases as E                                               # noqa: E402
import pol_cases as P                                                  # noqa: E402
import vol_reg_cases as R                                              # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401
from same_bits import bits, mismatch, record_of                        # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'eht_same_bits.json')
SAMPLE = 32
LIMIT = 48 << 10                           # bytes: well below tests/golden/step_same_bits.json

CLS_EXTRA = [('w300', Sx, dt) for Sx in T.BY_NAME['w300'].cls_Sx for dt in ('amp', 'cphase+logcamp')]
POL_EXTRA = [('w300', Sx, dt) for Sx in (3, 4) for dt in ('pvis', 'm')]
CASES = (['uv/%s/%d' % p for p in T.UV_PARAMS]
         + ['cls/%s/%d/%s' % (p + (T.CLS_DTYPE,)) for p in T.CLS_PARAMS] + ['cls/%s/%d/%s' % p for p in CLS_EXTRA]
         + ['pol/%s/%d/%s' % (p + (T.POL_DTYPE,)) for p in T.POL_PARAMS] + ['pol/%s/%d/%s' % p for p in POL_EXTRA]
         + ['vol/%s' % n for n in R.ALL_CASES])


def _uv(device, name, Sx):
    from bhnerf_amd import engine
    c, d = T.BY_NAME[name], T.uv(name, Sx)
    images = torch.as_tensor(d['images'], device=device)
    out = {'vis': bits(torch.view_as_real(E.operator(d, 'vis').observe(d['images'])))}
    for dtype in c.uv:
        target, sigma = d['data'][dtype]
        loss, dimg = engine.chi2_eht(images, E.operator(d, dtype), target, sigma, 1.0, dtype, want_grad=True)
        alone, none = engine.chi2_eht(images, E.operator(d, dtype), target, sigma, 1.0, dtype, want_grad=False)
        assert none is None and dimg.shape == images.shape
        out.update({dtype + ' loss': bits(loss), dtype + ' dimages': bits(dimg), dtype + ' loss forward only': bits(alone)})
        assert np.array_equal(out[dtype + ' loss'], out[dtype + ' loss forward only']), (name, Sx, dtype)
    return out


def _terms(device, d, op, packed, scale, dtype):
    from bhnerf_amd import engine
    images = torch.as_tensor(d['images'], device=device)
    loss, dimg = engine.chi2_eht(images, op, packed[0], packed[1], scale, dtype, want_grad=True)
    out = {'terms': bits(op.last_terms), 'dimages': bits(dimg)}
    assert dimg.shape == images.shape and np.array_equal(bits(loss), out['terms'][:1])
    return out


def _vol(device, name):
    from bhnerf_amd import engine, regularization
    c = R.make_case(name)
    coords = np.array(np.meshgrid(*[h * np.arange(n) for h, n in zip(c['spacing'], c['e'].shape[1:])], indexing='ij'))
    op = regularization.VolumePrior(coords=coords, weights=dict(zip(R.TERMS, c['weights'])), eps=c['eps'], normalize=False)
    e = torch.as_tensor(np.ascontiguousarray(c['e']), device=device)
    loss, dvol = engine.chi2_volume(e, op, c['scale'], mask=c['mask'])
    assert dvol.shape == e.shape and torch.equal(loss, op.last_terms[:1])
    return {'terms': bits(op.last_terms), 'per_volume': bits(op.last_per_volume), 'dvolumes': bits(dvol)}


def run_case(device, key):
    """{array name: uint32 bits} of one case of CASES."""
    lib, _, rest = key.partition('/')
    if lib == 'vol':
        return _vol(device, rest)
    name, Sx, dtype = (rest.split('/') + [None])[:3]
    Sx = int(Sx)
    if lib == 'uv':
        return _uv(device, name, Sx)
    if lib == 'cls':
        d = T.cls(name, Sx)
        return _terms(device, d, K.operator(d, dtype, K.WEIGHTS), K.packed(d, dtype), T.CLS_SCALE, dtype)
    d = T.pol(name, Sx)
    return _terms(device, d, P.operator(d, P.WEIGHTS), P.packed(d, dtype), P.SCALE, dtype)


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_record_is_whole(recorded):
    assert sorted(recorded['cases']) == sorted(CASES) and os.path.getsize(FIXTURE) <= LIMIT


@pytest.mark.parametrize('key', CASES)
def test_terms_keep_their_bits(dev, recorded, key):
    out, want = run_case(dev, key), recorded['cases'][key]
    assert sorted(out) == sorted(want), (key, sorted(out), sorted(want))
    bad = [m for m in (mismatch(k, out[k], want[k]) for k in sorted(out)) if m is not None]
    assert not bad, '%s: %s' % (key, ' | '.join(bad))


def record(path):
    """Every case twice on this device; a case whose two runs agree bit for bit is written, the others are reported."""
    device = torch.device('cuda:0')
    cases, unpinned = {}, []
    for key in CASES:
        a, b = run_case(device, key), run_case(device, key)
        same = sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
        print('%-40s %s' % (key, 'reproducible' if same else 'NOT REPRODUCIBLE'), flush=True)
        if same:
            cases[key] = {k: record_of(v, SAMPLE) for k, v in a.items()}
        else:
            unpinned.append(key)
    with open(path, 'w') as f:
        json.dump(dict(cases=cases), f, indent=0, sort_keys=True)
        f.write('\n')
    size = os.path.getsize(path)
    print('recorded %d of %d cases -> %s (%d bytes); not pinned: %s' % (len(cases), len(CASES), path, size, unpinned or 'none'))
    assert size <= LIMIT, 'the fixture is larger than it may be: lower SAMPLE (the SHA-256 stays authoritative)'


if __name__ == '__main__':
    if sys.argv[1:2] != ['--record'] or len(sys.argv) > 3:
        sys.exit('usage: python tests/test_gpu_eht_same_bits.py --record [FILE]   (rewrites %s, or FILE)' % FIXTURE)
    record(sys.argv[2] if len(sys.argv) == 3 else FIXTURE)
