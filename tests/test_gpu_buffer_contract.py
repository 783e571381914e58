"""GPU tests of the caller-owned-buffer contract of the fused and general MLP entry points (include/bhnerf_hip.h: the caller allocates
`packed`, `emission`, `images`, `dparams` and `workspace`; what they hold on entry is irrelevant; nothing outside the sizes that
bhn_packed_bytes and bhn_render_bwd_workspace_bytes report is written).  Every other GPU test reaches these kernels through
engine.FusedPredictor, whose torch.empty buffers are usually zero in a fresh process and are followed by the caching allocator's own
memory: a kernel that relies on zeros, or stores a few hundred bytes past the end, passes there.

Here the C ABI is called directly (only the geometry comes from pred.geometry / geom.c_struct_fused / eng._frames), and every buffer the
library writes is a slice, of exactly the size the ABI names, of a larger uint8 allocation: GUARD = 1 MiB before and behind it (a
multiple of 4096: the slice keeps the allocator's alignment), slice and guards pre-filled with the case's fill byte --
    0x00  the baseline (its guards hold 0xA5, so that a stray zero shows);
    0xFF  NaN as f32, as bf16 and as e4m3, every relu / mask bit set;
    0x7F  0x7F7F7F7F = 3.39e38 as f32, the same magnitude as bf16, NaN as e4m3.
Per case (buffer_contract_cases.CASES: one per backward path, on the ray sets that reach the tails) and fill byte, on fresh buffers:
bhn_pack_weights, bhn_predict_fwd, bhn_render_fwd, bhn_render_fwd_train, bhn_render_bwd_tape, bhn_render_bwd all at once (in a fresh,
filled workspace of the queried size) and bhn_render_bwd in a workspace of the LEAST size the call accepts (found by bisection over
multiples of 256 bytes; a refused call returns BHN_EWORKSPACE and launches nothing), where the fused paths run one frame per pass.

Asserted: the path (gpu_support.assert_path with the groups per tile; the ray set's remainders); every guard byte and every read-only input
unchanged; emission, both images and all gradients BITWISE equal across the three fills (the kernels are bitwise reproducible; an
element nobody writes is NaN under 0xFF); and, on the 0x00 run, the results against mlp_reference.linear_reference: f32 against
the float64 oracle (1e-5 of the maximum for emission and images -- times 2^(deg-5) for the images of the posenc-degree-10 case, as
test_shapes_outside_the_fused_kernels -- and mlp_bounds' GTOL / L2TOL for the gradient against oracle_torch.grad_linear), bf16
against the oracle_bf16 emulator of the recipe that ran inside 4x the figures observed on the MI355X (OBSERVED), capped at
mlp_bounds' CAPS['random']; the 8-bit tape against the float64 oracle at test_tape8_mode_gradient's bounds.  ReLU ties are
adjudicated by mlp_bounds.held_or_adjudicated.  The taped and the recomputed gradient relate as the older tests hold them:
bitwise on every path, the images of the training forward bitwise on the
general path and within test_taped_training_path_equals_recompute_path's rtol 1e-6 / atol 1e-7 of the maximum on the fused ones; the
least-workspace gradient equals the all-at-once one per tensor at test_gpu_frame_chunks' rtol 1e-5 / atol 1e-6 of the tensor's maximum.
The 8-bit tape's chunked call calibrates on frame 0 only, so it is held to the float64 oracle, not to the all-at-once call (as
test_tape8_chunked_backward_calibrating_and_second_call explains); its first tape call calibrates, the second does not, and both are
compared across the fills."""
import ctypes as C

import numpy as np
import pytest
import torch

import buffer_contract_cases as bc
from buffer_contract_cases import CASES, problem, reference
from gpu_support import assert_path, dev, device_setup, expected_flags  # noqa: F401
from guarded import Guarded
from mlp_bounds import (GTOL, IMG_TOL, L2TOL, TOL, capped_bounds, caps_of, first_difference, held_or_adjudicated, l2err, maxerr as mx, tensor_l2,
                        tensor_label)
from mlp_problems import tensor_cuts

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
FILLS = (0x00, 0xFF, 0x7F)
BHN_EWORKSPACE = 4

# Observed on the MI355X against the emulator, per bf16 case, as every case prints them: (image error / maximum, emission relative L2,
# relative L2 of the whole gradient = the worst of the taped, recomputed and least-workspace routes, worst relative L2 of one kernel /
# bias tensor).  The bound of a case is 4x its own figure, capped at CAPS['random'] -- except for the cases of CAPS_ONLY.
OBSERVED = {
    '4x128 S0 tiny':            (6.53e-05, 1.76e-04, 1.08e-03, 3.72e-03),      # 150 points: held to the caps (CAPS_ONLY)
    '4x128 S3 x12':             (1.49e-04, 7.73e-05, 2.18e-05, 6.27e-05),
    '4x128 S0 deg0 ragged':     (5.80e-05, 6.01e-05, 1.84e-06, 4.38e-06),
    '4x100 S2 ragged':          (2.42e-05, 4.75e-05, 1.05e-04, 2.54e-04),
    '4x128 S0 compacted pad':   (9.68e-05, 7.84e-05, 3.30e-05, 9.95e-05),
    '4x256 S3 ragged':          (1.46e-04, 1.43e-04, 2.06e-04, 5.38e-04),
    '4x256 S0 tiny':            (7.93e-06, 4.00e-05, 1.60e-05, 2.29e-05),      # 150 points: held to the caps (CAPS_ONLY)
    '6x256 S1 compacted':       (2.37e-04, 1.72e-04, 2.57e-04, 5.10e-04),
    '6x64 S2 ragged':           (6.26e-05, 7.64e-05, 2.43e-04, 4.37e-04),
    '2x256 S0 ragged':          (4.52e-05, 4.13e-05, 1.56e-05, 3.08e-05),
    '4x320 S2 deg6 ragged':     (1.10e-04, 2.40e-04, 2.95e-04, 1.21e-03),
}
# 150 points: one flipped bf16 rounding moves the figure of such a case, so 4x its own figure means nothing; these are held to the caps
# (the emission, which has no cap of its own, to the image cap: an image is a weighted sum of emissions)
CAPS_ONLY = {'4x128 S0 tiny', '4x256 S0 tiny'}
FIELDS = ('image', 'emission', 'grad', 'tensor')


def bf16_bounds(name):
    cap = caps_of('random', CASES[name][4])
    if name in CAPS_ONLY or name not in OBSERVED:          # (not in OBSERVED: a new case's first, measuring run)
        return dict(cap, emission=cap['image'])
    return capped_bounds(FIELDS, OBSERVED[name], cap)


def setup(dev, name, drop=None):
    """Predictor, engine, geometry and the read-only inputs of a case (drop: the tie adjudication's ray samples, Doppler weight 0)."""
    prob = problem(name)
    pred, eng, geom, params, tM0 = device_setup(prob['g'], CASES[name][2], dev, drop=drop)
    dimg = prob['dimg'].float().to(dev).contiguous()
    assert tuple(dimg.shape) == (prob['B'], geom.Sx, geom.R)
    k = geom.compact
    arrays = dict(coords=geom.coords, Omega=geom.Omega, t_geo=geom.t_geo, w=geom.w, dom=geom.dom) if k is None else \
        {n: k[n] for n in ('x', 'y', 'z', 'Omega', 't_geo', 'w', 'dom', 'ray')}
    inputs = dict(arrays, params=params, dimages=dimg, tM0=tM0)
    return dict(prob=prob, eng=eng, geom=geom, params=params, tM0=tM0, dimg=dimg, inputs=inputs,
                npts=geom.P if k is None else k['n_pad'], general=eng.general)


def least_workspace(dev, su):
    """The least workspace_bytes bhn_render_bwd accepts for this case (a multiple of 256), by bisection: a refused call returns
    BHN_EWORKSPACE and launches nothing; an accepted one runs inside a scratch workspace of the upper end's size."""
    from bhnerf_amd import _hip
    lib, eng, geom = _hip.lib(), su['eng'], su['geom']
    q = lambda nb, P: int(lib.bhn_render_bwd_workspace_bytes(C.byref(eng.model), eng.mode, nb, P, 0))
    one = q(1, geom.P_eff)
    hi = max(one, q(1, 16 * 32)) if su['general'] else one       # the general path asks for 16 groups of tape, not for a frame's
    assert hi > 0 and hi % 256 == 0
    ws = torch.empty((hi,), dtype=torch.uint8, device=dev)
    out = torch.empty((eng.nparams,), dtype=torch.float32, device=dev)
    gs, fs = geom.c_struct_fused(), eng._frames(su['tM0'])
    mode = eng.mode | (_hip.BHN_T8_CALIBRATE if eng.mode == _hip.BHN_BF16_T8 else 0)
    calls = [0]

    def accepted(nbytes):
        calls[0] += 1
        rc = lib.bhn_render_bwd(C.byref(eng.model), mode, _hip.ptr(su['packed0']), C.byref(gs), C.byref(fs), _hip.ptr(su['dimg']),
                                _hip.ptr(out), _hip.ptr(ws), nbytes, _hip.stream_ptr(dev))
        assert rc in (0, BHN_EWORKSPACE), (rc, lib.bhn_last_error())
        assert rc == 0 or b'workspace' in lib.bhn_last_error()
        return rc == 0
    assert accepted(hi) and not accepted(256)
    lo, up = 1, hi // 256                    # in units of 256 bytes: lo refused, up accepted
    while up - lo > 1:
        mid = (lo + up) // 2
        lo, up = (lo, mid) if accepted(256 * mid) else (mid, up)
    least = 256 * up
    # one frame per pass at that size (fused paths): the recorded-tape entry point, which needs the tape of ALL its frames at once,
    # refuses the first TWO frames in `least` bytes (BHN_EWORKSPACE before anything is launched)
    two_refused = None
    if not su['general']:
        f2 = _hip.bhn_frames(2, su['tM0'].data_ptr(), None)
        img = torch.empty((2, geom.Sx, geom.R), dtype=torch.float32, device=dev)
        two_refused = lib.bhn_render_fwd_train(C.byref(eng.model), eng.mode, _hip.ptr(su['packed0']), C.byref(gs), C.byref(f2), _hip.ptr(img),
                                               _hip.ptr(ws), least, _hip.stream_ptr(dev)) == BHN_EWORKSPACE
    torch.cuda.synchronize()
    assert calls[0] <= 24
    return least, one, q, two_refused


def run_sequence(dev, name, fill, su, least):
    """The seven calls of one case on fresh buffers filled with `fill` -> (outputs as numpy arrays, list of contract violations)."""
    from bhnerf_amd import _hip
    lib, eng, geom, prob = _hip.lib(), su['eng'], su['geom'], su['prob']
    B, st = prob['B'], _hip.stream_ptr(dev)
    M, gs, fs = C.byref(eng.model), geom.c_struct_fused(), eng._frames(su['tM0'])
    G, F = C.byref(gs), C.byref(fs)
    t8 = eng.mode == _hip.BHN_BF16_T8
    cal = eng.mode | (_hip.BHN_T8_CALIBRATE if t8 else 0)
    before = {k: v.clone() for k, v in su['inputs'].items()}
    ws_full = int(lib.bhn_render_bwd_workspace_bytes(M, eng.mode, B, geom.P_eff, 0))
    assert ws_full > 0
    mk = lambda label, n: Guarded(label, n, fill, dev, guard=GUARD, guard_fill=0xA5 if fill == 0x00 else None)
    nimg, npar = B * geom.Sx * geom.R * 4, eng.nparams * 4
    bufs = dict(packed=mk('packed', int(lib.bhn_packed_bytes(M, eng.mode))), emission=mk('emission', B * su['npts'] * 4),
                images=mk('images of bhn_render_fwd', nimg), images_train=mk('images of bhn_render_fwd_train', nimg),
                ws_tape=mk('workspace of the training pair', ws_full), grad_tape=mk('dparams of bhn_render_bwd_tape', npar),
                ws_rec=mk('workspace of bhn_render_bwd, all at once', ws_full), grad_rec=mk('dparams of bhn_render_bwd, all at once', npar),
                ws_least=mk('least workspace of bhn_render_bwd', least), grad_least=mk('dparams of bhn_render_bwd, least workspace', npar))
    if t8:
        bufs['grad_tape2'] = mk('dparams of the second (non-calibrating) bhn_render_bwd_tape', npar)
    b = bufs
    P, dI = b['packed'].ptr, _hip.ptr(su['dimg'])
    check = _hip.check
    check(lib.bhn_pack_weights(M, eng.mode, _hip.ptr(su['params']), P, st))
    check(lib.bhn_predict_fwd(M, eng.mode, P, G, F, b['emission'].ptr, st))
    check(lib.bhn_render_fwd(M, eng.mode, P, G, F, b['images'].ptr, st))
    check(lib.bhn_render_fwd_train(M, eng.mode, P, G, F, b['images_train'].ptr, b['ws_tape'].ptr, ws_full, st))
    check(lib.bhn_render_bwd_tape(M, cal, P, G, F, dI, b['grad_tape'].ptr, b['ws_tape'].ptr, ws_full, st))
    if t8:
        check(lib.bhn_render_bwd_tape(M, eng.mode, P, G, F, dI, b['grad_tape2'].ptr, b['ws_tape'].ptr, ws_full, st))
    check(lib.bhn_render_bwd(M, cal, P, G, F, dI, b['grad_rec'].ptr, b['ws_rec'].ptr, ws_full, st))
    check(lib.bhn_render_bwd(M, cal, P, G, F, dI, b['grad_least'].ptr, b['ws_least'].ptr, least, st))
    torch.cuda.synchronize()
    where = 'case %r, fill 0x%02X: ' % (name, fill)
    bad = [where + m for m in (v.disturbed() for v in bufs.values()) if m]
    for k, v in su['inputs'].items():
        if not torch.equal(v, before[k]):
            i = int(torch.nonzero((v != before[k]).reshape(-1))[0])
            bad.append(where + 'read-only input %s changed, first at element %d' % (k, i))
    out = {k: v.f32() for k, v in bufs.items() if not k.startswith('ws_') and k != 'packed'}
    return out, bad


_RUNS = {}


def evaluate(dev, name):
    """Everything the device does for a case, once: the least workspace, then the sequence under each of the three fills."""
    if name in _RUNS:
        return _RUNS[name]
    from bhnerf_amd import _hip
    su = setup(dev, name)
    eng = su['eng']
    su['packed0'] = torch.empty((int(_hip.lib().bhn_packed_bytes(C.byref(eng.model), eng.mode)),), dtype=torch.uint8, device=dev)
    _hip.check(_hip.lib().bhn_pack_weights(C.byref(eng.model), eng.mode, _hip.ptr(su['params']), _hip.ptr(su['packed0']), _hip.stream_ptr(dev)))
    least, one, q, two_refused = least_workspace(dev, su)
    runs, bad = {}, []
    for fill in FILLS:
        runs[fill], b = run_sequence(dev, name, fill, su, least)
        bad += b
    _RUNS[name] = dict(su=su, least=least, one=one, q=q, two_refused=two_refused, runs=runs, bad=bad)
    return _RUNS[name]


@pytest.mark.parametrize('name', list(CASES))
def test_path_and_least_workspace(dev, name):
    """The case runs the path it is listed under, on a ray set with the listed remainders, and the least workspace bhn_render_bwd
    accepts is no larger than the one-frame query (general path: it is slabs + 16 groups of tape, whatever a frame holds)."""
    depth, width, mode, S, deg, rays, recipe, nwf = CASES[name]
    r = evaluate(dev, name)
    su, q = r['su'], r['q']
    geom = su['geom']
    npts, groups, m8, m12, last = bc.RAGGED[rays]
    compact = rays.startswith('compacted')
    flags, _ = assert_path(name, su['eng'], geom, mode, recipe, recipe.startswith('general'), compact=compact, tile_groups=nwf)
    assert flags['drop_ga'] == expected_flags(recipe)['drop_ga'], (name, flags)      # (here on the general path too, which assert_path leaves open)
    assert geom.P_eff == 32 * groups
    assert (geom.compact['n'] if compact else geom.P) == npts and npts % 32 == last % 32
    assert (groups % 8, groups % 12) == (m8, m12)
    assert su['npts'] == (32 * groups if compact else npts)
    least, one = r['least'], r['one']
    print('\n[buffer contract] %-26s %-11s %5d groups/frame  workspace: all frames %d, one-frame query %d, least accepted %d (%d under the query)'
          % (name, recipe, groups, q(su['prob']['B'], geom.P_eff), one, least, one - least))
    if su['general']:
        assert least == (q(1, 16 * 32) + 255) // 256 * 256, (name, least, q(1, 16 * 32))
    else:
        assert least <= one, (name, least, one)
        assert r['two_refused'], (name, 'the tape of two frames fits the least workspace: not one frame per pass')


@pytest.mark.parametrize('name', list(CASES))
def test_guard_bands_and_independence_of_buffer_contents(dev, name):
    r = evaluate(dev, name)
    assert not r['bad'], '\n'.join(r['bad'])
    base = r['runs'][0x00]
    for key, a in base.items():
        assert np.isfinite(a).all(), 'case %r, fill 0x00, %s: element %d is not finite' % (name, key, int(np.nonzero(~np.isfinite(a.reshape(-1)))[0][0]))
        for fill in FILLS[1:]:
            d = first_difference(r['runs'][fill][key], a)
            assert d is None, 'case %r, %s: fill 0x%02X differs from fill 0x00, first at element %d (%r vs %r)' % ((name, key, fill) + d)


def compare(name, out, ref, su):
    """The figures of one run against a reference."""
    prob, geom = su['prob'], su['geom']
    B = prob['B']
    e = out['emission'].reshape(B, -1).astype(np.float64)
    e_ref = ref['emission']
    if geom.compact is not None:
        n = geom.compact['n']
        assert not e[:, n:].any(), (name, 'emission of the dom = 0 padding points')
        e, e_ref = e[:, :n], e_ref[:, bc.domain_mask(prob).reshape(-1)]
    cuts = tensor_cuts(prob['g'])
    gref = ref['grad']
    routes = {k: out[k].astype(np.float64) for k in ('grad_tape', 'grad_rec', 'grad_least')}
    tens = np.max([tensor_l2(g, gref, cuts, False) for g in routes.values()], axis=0)
    return dict(emission_max=mx(e, e_ref), emission=l2err(e, e_ref),
                image=max(mx(out[k].reshape(ref['images'].shape).astype(np.float64), ref['images']) for k in ('images', 'images_train')),
                grad=max(l2err(g, gref) for g in routes.values()), gmax=max(mx(g, gref) for g in routes.values()),
                tensor=max(tens), worst=int(np.argmax(tens)))


@pytest.mark.parametrize('name', list(CASES))
def test_results_against_reference_and_between_routes(dev, name):
    depth, width, mode, S, deg, rays, recipe, nwf = CASES[name]
    r = evaluate(dev, name)
    su, out = r['su'], r['runs'][0x00]
    general = su['general']
    # ---- between the routes
    d = first_difference(out['grad_tape'], out['grad_rec'])
    if mode != 'bf16_t8':
        assert d is None, 'case %r: taped and recomputed gradient differ, first at element %d (%r vs %r)' % ((name,) + d)
    a, b_ = out['images_train'], out['images']
    if general:
        assert first_difference(a, b_) is None, (name, 'images of the training forward', first_difference(a, b_))
    else:
        assert np.allclose(a, b_, rtol=1e-6, atol=1e-7 * float(np.abs(b_).max())), (name, 'images of the training forward')
    cuts = tensor_cuts(su['prob']['g'])
    vs_full = 0.0
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        x, y = out['grad_least'][c0:c1].astype(np.float64), out['grad_rec'][c0:c1].astype(np.float64)
        vs_full = max(vs_full, float((np.abs(x - y) / (1e-6 * np.abs(y).max() + 1e-5 * np.abs(y))).max()))
    if mode != 'bf16_t8':
        assert vs_full <= 1.0, 'case %r: least-workspace gradient vs all at once: %.3g of the bound' % (name, vs_full)
    # ---- against the reference
    ref_recipe = recipe if mode == 'bf16' else None
    if mode == 'f32':
        k = max(1.0, 2.0 ** (deg - 5)) if deg == 10 else 1.0
        ok = lambda f: f['emission_max'] < 1e-5 and f['image'] < 1e-5 * k and f['gmax'] < GTOL['f32'] and f['grad'] < L2TOL['f32']
    elif mode == 'bf16_t8':
        ok = lambda f: f['emission_max'] < TOL['bf16'] and f['image'] < IMG_TOL['bf16'] and f['gmax'] < GTOL['bf16'] and f['grad'] < L2TOL['bf16']
    else:
        bnd = bf16_bounds(name)
        ok = lambda f: all(f[key] < bnd[key] for key in FIELDS)
    f = compare(name, out, reference(name, ref_recipe), su)
    line = lambda f: ('vs %s: image %.2e  emission max %.2e L2 %.2e  gradient L2 %.2e max %.2e  worst tensor %.2e (%s)   least workspace vs all at '
                      'once %.2f of the bound' % ('emulator' if ref_recipe else 'f64 oracle', f['image'], f['emission_max'], f['emission'], f['grad'],
                                                  f['gmax'], f['tensor'], tensor_label(f['worst']), vs_full))
    print('\n[buffer contract] %-26s %-11s %s' % (name, recipe, line(f)))
    if mode == 'bf16':
        print("    %-28s(%.2e, %.2e, %.2e, %.2e)," % (repr(name) + ':', f['image'], f['emission'], f['grad'], f['tensor']))

    def rerun(ties):
        su2 = setup(dev, name, drop=ties)
        su2['packed0'] = su['packed0']
        out2, bad2 = run_sequence(dev, name, 0x00, su2, r['least'])
        f2 = compare(name, out2, reference(name, ref_recipe, drop=ties), su2)
        print('    without the tied ray samples: %s' % line(f2))
        return dict(f2, bad=bad2)
    good, _ = held_or_adjudicated(name, f, ok, lambda: reference(name, ref_recipe, want_ties=True), rerun, lambda f2: not f2['bad'])
    assert good, (name, line(f))
