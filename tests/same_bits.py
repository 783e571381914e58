"""What the same-bits guards share (test_gpu_w256_same_bits with tests/golden/w256_same_bits.json, test_gpu_step_same_bits with
tests/golden/step_same_bits.json; the records are held to their rules on the CPU by test_step_cases_cpu): float32 arrays as uint32
bits, the record of an array -- its length, a SHA-256 and a strided sample --, the comparison of an array with its record and the
message it gives, the problem and the chi^2 targets of a case, and run_case: two gradient steps of a case on a fresh predictor.
No test here, and no CUDA call at import.

A case is a dict: depth, S (Stokes planes, 0: none), shape (rays H, rays W, samples, frames), domain (scale, rmin, rmax, z_width),
dt ('full' or 'lc'), cap (frames of tape the workspace is capped to, None: all) and, where they differ from the width-256 guard's,
mode ('bf16'), width (256), deg (posenc degree, 3), do_skip (True)."""
import ctypes as C
import hashlib

import numpy as np
import torch

from mlp_problems import random_problem_inputs, without_samples

SAMPLE = 1024
CUS = 256
ARRAYS = ('loss', 'images', 'grad', 'params', 'adam_m', 'adam_v')


def bits(t):
    """A float32 tensor / array as a flat uint32 numpy array."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def sample_of(u, sample=SAMPLE):
    stride = max(1, -(-u.size // sample))
    return stride, u[::stride][:sample]


def record_of(u, sample=SAMPLE):
    stride, s = sample_of(u, sample)
    return dict(n=int(u.size), sha256=hashlib.sha256(u.tobytes()).hexdigest(), stride=stride, sample=''.join('%08x' % v for v in s))


def sample_bits(rec):
    """The sampled elements of a record as uint32."""
    return np.array([int(rec['sample'][8 * i:8 * i + 8], 16) for i in range(len(rec['sample']) // 8)], dtype=np.uint32)


def mismatch(k, u, want):
    """None when the uint32 array `u` is the array the record `want` was taken from (length and SHA-256), else the message: the first
    sampled element that differs, or that every sampled element is equal (the difference lies between the samples)."""
    n = int(u.size)
    if n == want['n'] and hashlib.sha256(u.tobytes()).hexdigest() == want['sha256']:
        return None
    msg = '%s: %d values (recorded %d), sha256 differs' % (k, n, want['n'])
    if n == want['n']:
        stride, ref = want['stride'], sample_bits(want)
        s = u[::stride][:ref.size]
        d = np.nonzero(s != ref)[0]
        if d.size:
            i = int(d[0])
            msg += '; first differing sampled element: index %d, %08x (%.9g) against the recorded %08x (%.9g); %d of %d sampled differ' % (
                i * stride, s[i], s[i:i + 1].view(np.float32)[0], ref[i], ref[i:i + 1].view(np.float32)[0], d.size, s.size)
        else:
            msg += '; every sampled element (stride %d) is equal' % stride
    return msg


def mismatches(out, want, arrays=ARRAYS):
    """The messages of the arrays of `out` ({name: uint32 bits}) that are not the recorded ones."""
    return [m for m in (mismatch(k, out[k], want[k]) for k in arrays) if m is not None]


def first_difference(a, b):
    """None when two runs of a case gave the same bits, else (array name, first differing flat index, the two words)."""
    for k in ARRAYS:
        if a[k].size != b[k].size:
            return k, -1, a[k].size, b[k].size
        d = np.nonzero(a[k] != b[k])[0]
        if d.size:
            return k, int(d[0]), int(a[k][d[0]]), int(b[k][d[0]])
    return None


def case_problem(c):
    """mlp_problems.random_problem_inputs of a case."""
    return random_problem_inputs(c.get('width', 256), c['depth'], c['S'], c.get('deg', 3), shape=c['shape'], domain=c['domain'],
                                 do_skip=c.get('do_skip', True))


def case_targets(c, prob):
    """[target, sigma, offset] of a case's chi^2: the problem's own per pixel ('full'), or per frame and Stokes plane ('lc')."""
    if c['dt'] == 'full':
        return [prob[k] for k in ('target', 'sigma', 'offset')]
    B, S = c['shape'][3], c['S']
    rng = np.random.default_rng(41)
    return [rng.uniform(0, 1e-1, (B, S)), rng.uniform(0.5, 2.0, (B, S)), np.zeros((B, S))]


def run_case(dev, name, c, check, first=None, drop=None, steps=2):
    """`steps` gradient steps of the case `c` on a fresh predictor -> {array name: uint32 bits}.  check(name, eng, geom, groups, flags)
    asserts the layout and the path the case is listed for; render == render_train is asserted here, on the parameters the steps
    left.  first: a dict that receives what the FIRST step gave on the parameters before it -- loss, images and gradient as float32
    arrays (what the reference of a case is compared with) -- and the tape_info flags.  drop: (H, W, G) bool, ray samples taken out
    of the problem (Doppler weight 0: the ReLU-tie adjudication)."""
    from bhnerf_amd import _hip, engine as E, network, units
    from conftest import golden_tree
    from gpu_support import predictor_of, ray_args
    from oracle import oracle_np as onp
    H, Wd, G, B = c['shape']
    prob = case_problem(c)
    g, S = without_samples(prob['g'], drop), c['S']
    pred, rt = predictor_of(g, c.get('mode', 'bf16'), dev, c.get('do_skip')), ray_args(g)
    eng = pred.engine()
    geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], rt['J'] if S else None, rt['g'], rt['dtau'], rt['Sigma'])
    groups = (geom.P_eff + 31) // 32
    if c['cap'] is not None:
        eng.max_workspace_bytes = int(_hip.lib().bhn_render_bwd_workspace_bytes(C.byref(eng.model), eng.mode, c['cap'], geom.P_eff, dev.index or 0))
        assert not eng.fits_tape(B, geom.P_eff) and eng.tape_group(B, geom.P_eff) == c['cap'] < B, name
    else:
        assert eng.fits_tape(B, geom.P_eff), name
    flags = eng.tape_info(groups)['flags']
    check(name, eng, geom, groups, flags)
    tg = case_targets(c, prob)
    state = pred.init_state(network.ParamTree(golden_tree(g)), num_iters=2, lr_init=1e-3, lr_final=1e-4)
    for i in range(steps):
        loss, state, images = network.gradient_step_image(
            state, units.hr, c['dt'], tg[0], tg[1], tg[2], g['t_frames'], rt['coords'], rt['Omega'], rt['J'], rt['g'], rt['dtau'],
            rt['Sigma'], rt['t_start_obs'], rt['t_geos'], rt['t_injection'], 1.0)
        if i == 0 and first is not None:
            first.update(loss=loss.cpu().numpy().copy(), images=images.cpu().numpy().copy(),
                         grad=state.grad[:eng.nparams].cpu().numpy().copy(), flags=dict(flags))
    out = dict(loss=bits(loss), images=bits(images), grad=bits(state.grad[:eng.nparams]), params=bits(state.flat), adam_m=bits(state.m),
               adam_v=bits(state.v))
    assert state.step == steps and np.isfinite(out['loss'].view(np.float32)).all() and out['grad'].any() and out['images'].any(), name
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
