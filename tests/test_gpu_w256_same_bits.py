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
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_tree
from gpu_support import dev, predictor_of, ray_args  # noqa: F401
from mlp_problems import RANDOM_PROBLEM_DOMAIN, RANDOM_PROBLEM_SHAPE, random_problem_inputs

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'w256_same_bits.json')
ALL_ACTIVE = (8.0, 0.0, np.inf, np.inf)
SAMPLE = 1024
CUS = 256
ARRAYS = ('loss', 'images', 'grad', 'params', 'adam_m', 'adam_v')
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


def bits(t):
    """A float32 tensor / array as a flat uint32 numpy array."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def sample_of(u):
    stride = max(1, -(-u.size // SAMPLE))
    return stride, u[::stride][:SAMPLE]


def record_of(u):
    stride, s = sample_of(u)
    return dict(n=int(u.size), sha256=hashlib.sha256(u.tobytes()).hexdigest(), stride=stride, sample=''.join('%08x' % v for v in s))


def run_case(dev, name):
    """Two gradient steps of the case `name` on a fresh predictor -> {array name: uint32 bits}; asserts the layout the case is listed
    for and render == render_train on the parameters the two steps left."""
    from bhnerf_amd import _hip, engine as E, network, units
    from oracle import oracle_np as onp
    c = CASES[name]
    H, Wd, G, B = c['shape']
    prob = random_problem_inputs(256, c['depth'], c['S'], 3, shape=c['shape'], domain=c['domain'])
    g, S = prob['g'], c['S']
    pred, rt = predictor_of(g, 'bf16', dev), ray_args(g)
    eng = pred.engine()
    geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], rt['J'] if S else None, rt['g'], rt['dtau'], rt['Sigma'])
    groups = (geom.P_eff + 31) // 32
    assert (groups, geom.compact is not None) == LAYOUT[name], (name, groups, geom.compact is not None)
    if geom.compact is not None:
        assert geom.compact['ray_span'] <= 2, (name, geom.compact['ray_span'])
    if c['cap'] is not None:
        eng.max_workspace_bytes = int(_hip.lib().bhn_render_bwd_workspace_bytes(C.byref(eng.model), eng.mode, c['cap'], geom.P_eff, dev.index or 0))
        assert not eng.fits_tape(B, geom.P_eff) and eng.tape_group(B, geom.P_eff) == c['cap'] < B, name
    else:
        assert eng.fits_tape(B, geom.P_eff), name
    flags = eng.tape_info(groups)['flags']
    assert not flags['general'] and not flags['fused128'] and flags['ga0_chain'] and flags['drop_ga'], (name, flags)
    if c['dt'] == 'full':
        tg = [prob[k] for k in ('target', 'sigma', 'offset')]
    else:                                   # light curves: one value per frame and Stokes plane
        rng = np.random.default_rng(41)
        tg = [rng.uniform(0, 1e-1, (B, S)), rng.uniform(0.5, 2.0, (B, S)), np.zeros((B, S))]
    state = pred.init_state(network.ParamTree(golden_tree(g)), num_iters=2, lr_init=1e-3, lr_final=1e-4)
    for _ in range(2):
        loss, state, images = network.gradient_step_image(
            state, units.hr, c['dt'], tg[0], tg[1], tg[2], g['t_frames'], rt['coords'], rt['Omega'], rt['J'], rt['g'], rt['dtau'],
            rt['Sigma'], rt['t_start_obs'], rt['t_geos'], rt['t_injection'], 1.0)
    out = dict(loss=bits(loss), images=bits(images), grad=bits(state.grad[:eng.nparams]), params=bits(state.flat), adam_m=bits(state.m),
               adam_v=bits(state.v))
    assert state.step == 2 and np.isfinite(out['loss'].view(np.float32)).all() and out['grad'].any() and out['images'].any(), name
    # the inference forward against the training forward, frame group by frame group
    tM0 = E.frame_offsets(g['t_frames'], rt['t_start_obs'], rt['t_injection'], onp.GM_C3_SGRA_HR, dev)
    eng.pack(state.flat)
    nb = c['cap'] or B
    for b0 in range(0, B, nb):
        infer = bits(eng.render(geom, tM0[b0:b0 + nb]))
        train = bits(eng.render_train(geom, tM0[b0:b0 + nb]))
        diff = np.nonzero(infer != train)[0]
        assert diff.size == 0, '%s frames %d..: render and render_train differ in %d of %d image values, first at %d (%08x / %08x)' % (
            name, b0, diff.size, infer.size, diff[0], infer[diff[0]], train[diff[0]])
    return out


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
    bad = []
    for k in ARRAYS:
        got = record_of(out[k])
        if got['sha256'] == want[k]['sha256'] and got['n'] == want[k]['n']:
            continue
        msg = '%s: %d values (recorded %d), sha256 differs' % (k, got['n'], want[k]['n'])
        if got['n'] == want[k]['n']:
            stride, s = sample_of(out[k])
            ref = np.array([int(want[k]['sample'][8 * i:8 * i + 8], 16) for i in range(len(want[k]['sample']) // 8)], dtype=np.uint32)
            d = np.nonzero(s != ref)[0]
            if d.size:
                i = int(d[0])
                msg += '; first differing sampled element: index %d, %08x (%.9g) against the recorded %08x (%.9g); %d of %d sampled differ' % (
                    i * stride, s[i], s[i:i + 1].view(np.float32)[0], ref[i], ref[i:i + 1].view(np.float32)[0], d.size, s.size)
            else:
                msg += '; every sampled element (stride %d) is equal' % stride
        bad.append(msg)
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
