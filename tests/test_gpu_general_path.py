"""GPU tests of the general MLP path (csrc/general_mlp.hip: posenc_deg 5 ... 10 or net_width 257 ... 512) at its kernels' own edge
shapes -- general_path_cases.CASES, one case per branch of the host rules (m-tiles per layer against the waves of a workgroup, the
strips of the weight-gradient kernels, NG = 4 / 2 of the bf16 kernels, the zero slots of the encoded inputs, ray_direct, the chunks
of the recomputing backward, zero-padded widths), both arithmetic modes.  tests/test_general_path_cases_cpu.py proves on the CPU that
every case has the property it is listed for.

Per case and mode the C ABI is called directly, on buffers of exactly the sizes the ABI names that are pre-filled with 0xFF (NaN as f32
and as bf16, every relu bit set: a read of a tape or slab slot nobody wrote shows up as NaN) between guard bands: bhn_pack_weights,
bhn_predict_fwd, bhn_render_fwd, bhn_render_fwd_train + bhn_render_bwd_tape, bhn_render_bwd all at once -- twice, on fresh buffers.
Asserted: the general path (gpu_support.assert_path); packed and workspace bytes equal to the restated layout; both images and both
gradients bitwise equal to each other, and everything bitwise equal on the second run (that includes `long 257` and the
direct layouts); emission, images and gradients against a reference outside the code under test (mlp_reference.linear_reference) --
  f32   the float64 oracle: images and emission 1e-5 max(1, 2^(deg-5)) of the maximum, gradient max-norm and relative L2
        2e-5 max(1, 2^(deg-5)) (gpu_support.check_general_path_problem's figures; octave i multiplies the f32 rounding of the warped
        coordinate by 2^i before the sine, and the emission feels that as the images do);
  bf16  oracle_bf16's emulator of the `general` recipe: mlp_bounds.caps_of('random', deg) -- images 5e-4 max(1, 2^(deg-5)), whole
        gradient 3e-3, worst tensor 6e-3 relative L2, the emission (relative L2) at the image cap.
No bound comes from the kernels; the figures every case prints are recorded in DESIGN.md 2 and bound nothing.  ReLU ties are adjudicated
by mlp_bounds.held_or_adjudicated (the CPU test holds the tied share of every case under a quarter).  A workspace 256 bytes under
slabs + min(tiles, 2) tiles of tape is refused with BHN_EWORKSPACE, outputs untouched.

Chunk sweep (general_path_cases.CHUNK_SWEEP: NG 4, NG 2, compacted): bhn_render_bwd in a workspace of slabs + k tiles of tape, k = 2, 3, 5
and the tile count minus one (chunks that cut frames, a short last chunk, twelve and more accumulating passes) -- per tensor within rtol 1e-5 /
atol 1e-6 of the tensor's maximum of the all-at-once gradient (test_gpu_frame_chunks' figures), bitwise equal when repeated."""
import ctypes as C

import numpy as np
import pytest
import torch

import buffer_contract_cases as bc
import general_path_cases as gp
from general_path_cases import CASES, MODES, bounds, case_layout, problem, reference
from gpu_support import assert_path, dev, lib, device_setup, ptr, stream_ptr  # noqa: F401
from guarded import Guarded
from mlp_bounds import expected_recipe, first_difference, held_or_adjudicated, l2err, maxerr as mx, tensor_l2, tensor_label
from mlp_problems import tensor_cuts

pytestmark = pytest.mark.gpu

FILL = 0xFF
BHN_EWORKSPACE = 4
PAIRS = [(n, m) for n in CASES for m in MODES]
IDS = ['%s %s' % p for p in PAIRS]


def setup(dev, name, mode, drop=None):
    """Engine, geometry and the read-only inputs of a case (drop: the tie adjudication's ray samples, Doppler weight 0)."""
    prob = problem(name)
    pred, eng, geom, params, tM0 = device_setup(prob['g'], mode, dev, drop=drop, do_skip=prob['do_skip'])
    dimg = prob['dimg'].float().to(dev).contiguous()
    assert tuple(dimg.shape) == (prob['B'], geom.Sx, geom.R)
    return dict(name=name, mode=mode, prob=prob, eng=eng, geom=geom, params=params, tM0=tM0, dimg=dimg,
                npts=geom.P if geom.compact is None else geom.compact['n_pad'])


def call_args(dev, su):
    eng, geom = su['eng'], su['geom']
    gs, fs = geom.c_struct_fused(), eng._frames(su['tM0'])
    return C.byref(eng.model), eng.mode, gs, fs, stream_ptr(dev)


def run_sequence(dev, lib, su):
    """The six calls of a case on fresh buffers filled with 0xFF -> (outputs as numpy arrays, list of disturbed guard bands)."""
    from bhnerf_amd import _hip
    eng, geom, B = su['eng'], su['geom'], su['prob']['B']
    M, mode, gs, fs, st = call_args(dev, su)
    G, F = C.byref(gs), C.byref(fs)
    ws_full = int(lib.bhn_render_bwd_workspace_bytes(M, mode, B, geom.P_eff, 0))
    assert ws_full == gp.workspace_bytes(su['name'], su['mode'], case_layout(su['name'])['total_tiles']), (su['name'], ws_full)
    mk = lambda label, n: Guarded(label, n, FILL, dev)
    nimg, npar = B * geom.Sx * geom.R * 4, eng.nparams * 4
    b = dict(packed=mk('packed', int(lib.bhn_packed_bytes(M, mode))), emission=mk('emission', B * su['npts'] * 4),
             images=mk('images of bhn_render_fwd', nimg), images_train=mk('images of bhn_render_fwd_train', nimg),
             ws_tape=mk('workspace of the training pair', ws_full), grad_tape=mk('dparams of bhn_render_bwd_tape', npar),
             ws_rec=mk('workspace of bhn_render_bwd', ws_full), grad_rec=mk('dparams of bhn_render_bwd', npar))
    P, dI, check = b['packed'].ptr, ptr(su['dimg']), _hip.check
    check(lib.bhn_pack_weights(M, mode, ptr(su['params']), P, st))
    check(lib.bhn_predict_fwd(M, mode, P, G, F, b['emission'].ptr, st))
    check(lib.bhn_render_fwd(M, mode, P, G, F, b['images'].ptr, st))
    check(lib.bhn_render_fwd_train(M, mode, P, G, F, b['images_train'].ptr, b['ws_tape'].ptr, ws_full, st))
    check(lib.bhn_render_bwd_tape(M, mode, P, G, F, dI, b['grad_tape'].ptr, b['ws_tape'].ptr, ws_full, st))
    check(lib.bhn_render_bwd(M, mode, P, G, F, dI, b['grad_rec'].ptr, b['ws_rec'].ptr, ws_full, st))
    torch.cuda.synchronize()
    bad = [m for m in (v.disturbed() for v in b.values()) if m]
    out = {k: v.f32().copy() for k, v in b.items() if not k.startswith('ws_') and k != 'packed'}
    return out, bad, b['packed']


_RUNS = {}


def evaluate(dev, lib, name, mode):
    """Everything the device does for a case and mode, once: the sequence twice, on fresh buffers."""
    if (name, mode) not in _RUNS:
        su = setup(dev, name, mode)
        try:
            first, bad1, packed = run_sequence(dev, lib, su)
            second, bad2, _ = run_sequence(dev, lib, su)
        except AssertionError:
            raise
        except Exception as e:          # a device error: nothing else of this module is launched on that device
            pytest.exit('case %r %s: %r' % (name, mode, e), returncode=3)
        su['packed'] = packed
        _RUNS[(name, mode)] = dict(su=su, first=first, second=second, bad=bad1 + bad2)
    return _RUNS[(name, mode)]


def compare(out, ref, su):
    """The figures of one run against a reference."""
    prob, geom = su['prob'], su['geom']
    e = out['emission'].reshape(prob['B'], -1).astype(np.float64)
    e_ref = ref['emission']
    if geom.compact is not None:
        n = geom.compact['n']
        assert not e[:, n:].any(), (su['name'], 'emission of the dom = 0 padding points')
        e, e_ref = e[:, :n], e_ref[:, bc.domain_mask(prob).reshape(-1)]
    cuts = tensor_cuts(prob['g'])
    gref = ref['grad']
    routes = {k: out[k].astype(np.float64) for k in ('grad_tape', 'grad_rec')}
    tens = np.max([tensor_l2(g, gref, cuts, False) for g in routes.values()], axis=0)
    img = max(mx(out[k].reshape(ref['images'].shape).astype(np.float64), ref['images']) for k in ('images', 'images_train'))
    return dict(emission_max=mx(e, e_ref), emission_l2=l2err(e, e_ref), image=img, grad=max(l2err(g, gref) for g in routes.values()),
                gmax=max(mx(g, gref) for g in routes.values()), tensor=max(tens), worst=int(np.argmax(tens)),
                layers=[tens[2 * i] for i in range(len(tens) // 2)])


def within(f, mode, bnd):
    if mode == 'f32':
        return f['emission_max'] < bnd['emission'] and f['image'] < bnd['image'] and f['gmax'] < bnd['gmax'] and f['grad'] < bnd['grad']
    return f['emission_l2'] < bnd['emission'] and f['image'] < bnd['image'] and f['grad'] < bnd['grad'] and f['tensor'] < bnd['tensor']


def line(f, mode):
    return ('vs %s: image %.2e  emission max %.2e L2 %.2e  gradient L2 %.2e max %.2e  worst tensor %.2e (%s)  per-layer dK L2 %s'
            % ('f64 oracle' if mode == 'f32' else 'emulator', f['image'], f['emission_max'], f['emission_l2'], f['grad'], f['gmax'], f['tensor'],
               tensor_label(f['worst']), ' '.join('%.1e' % v for v in f['layers'])))


@pytest.mark.parametrize('name,mode', PAIRS, ids=IDS)
def test_path_sizes_and_refusal(dev, lib, name, mode):
    """The case runs the general path on the layout the CPU test proves it has; the ABI's sizes are the restated ones; a workspace
    256 bytes under slabs + min(tiles, 2) tiles of tape is refused before anything is launched."""
    depth, width, deg, S, rays, B, do_skip, _ = CASES[name]
    r = evaluate(dev, lib, name, mode)
    su, L = r['su'], case_layout(name)
    eng, geom = su['eng'], su['geom']
    compact = rays.startswith('compacted')
    assert_path(name, eng, geom, mode, expected_recipe(depth, L['Wp'], True), True, compact=compact)
    assert eng.general and geom.P_eff == 32 * L['groups'] and geom.G == gp.RAY_SETS[rays][2]
    assert (geom.compact['ray_span'] if compact else None) == L['ray_span'], (name, L['ray_span'])
    assert (geom.compact['n'] if compact else geom.P) == gp.points_per_frame(name)
    M, m, gs, fs, st = call_args(dev, su)
    assert int(lib.bhn_packed_bytes(M, m)) == L['packed_bytes'][mode]
    least = gp.workspace_bytes(name, mode, min(L['total_tiles'], 2))
    ws = Guarded('workspace under the least size', least - 256, FILL, dev)
    grad = Guarded('dparams of the refused call', eng.nparams * 4, FILL, dev)
    rc = lib.bhn_render_bwd(M, m, su['packed'].ptr, C.byref(gs), C.byref(fs), ptr(su['dimg']), grad.ptr, ws.ptr, least - 256, st)
    torch.cuda.synchronize()
    assert rc == BHN_EWORKSPACE and b'workspace' in lib.bhn_last_error(), (name, rc, lib.bhn_last_error())
    assert grad.untouched() and ws.untouched() and not grad.disturbed() and not ws.disturbed(), (name, 'a refused call wrote')
    print('\n[general path] %-32s %-4s Wp %d Ep %d MTp %d on %d waves  NG %d (%d bytes of LDS)  %d groups, %d tiles  ray_direct %s'
          % (name, mode, L['Wp'], L['Ep'], L['MTp'], L['waves'], L['NG'], L['lds16'], L['groups'], L['total_tiles'], L['ray_direct']))


@pytest.mark.parametrize('name,mode', PAIRS, ids=IDS)
def test_routes_and_runs_are_bitwise_equal(dev, lib, name, mode):
    r = evaluate(dev, lib, name, mode)
    assert not r['bad'], '\n'.join(r['bad'])
    a = r['first']
    for key, v in a.items():
        assert np.isfinite(v).all(), 'case %r %s, %s: element %d is not finite' % (name, mode, key, int(np.nonzero(~np.isfinite(v.reshape(-1)))[0][0]))
        d = first_difference(r['second'][key], v)
        assert d is None, 'case %r %s, %s: the second run differs, first at element %d (%r vs %r)' % ((name, mode, key) + d)
    d = first_difference(a['images_train'], a['images'])
    assert d is None, 'case %r %s: images of the training forward differ, first at element %d (%r vs %r)' % ((name, mode) + d)
    d = first_difference(a['grad_tape'], a['grad_rec'])
    assert d is None, 'case %r %s: taped and recomputed gradient differ, first at element %d (%r vs %r)' % ((name, mode) + d)


@pytest.mark.parametrize('name,mode', PAIRS, ids=IDS)
def test_results_against_reference(dev, lib, name, mode):
    r = evaluate(dev, lib, name, mode)
    su, bnd = r['su'], bounds(name, mode)
    f = compare(r['first'], reference(name, mode), su)
    print('\n[general path] %-32s %-4s %s' % (name, mode, line(f, mode)))

    def rerun(ties):
        su2 = setup(dev, name, mode, drop=ties)
        out2, bad2, _ = run_sequence(dev, lib, su2)
        f2 = compare(out2, reference(name, mode, drop=ties), su2)
        print('    without the tied ray samples: %s' % line(f2, mode))
        return dict(f2, bad=bad2)
    good, _ = held_or_adjudicated('%s %s' % (name, mode), f, lambda f: within(f, mode, bnd), lambda: reference(name, mode, want_ties=True),
                                   rerun, lambda f2: not f2['bad'])
    assert good, (name, mode, line(f, mode), bnd)


@pytest.mark.parametrize('name,mode', [(n, m) for n in gp.CHUNK_SWEEP for m in MODES], ids=['%s %s' % (n, m) for n in gp.CHUNK_SWEEP for m in MODES])
def test_chunk_sweep(dev, lib, name, mode):
    r = evaluate(dev, lib, name, mode)
    su, L = r['su'], case_layout(name)
    eng, full = su['eng'], r['first']['grad_rec']
    M, m, gs, fs, st = call_args(dev, su)
    cuts = tensor_cuts(su['prob']['g'])
    total = L['total_tiles']
    for k in [total - 1 if k < 0 else k for k in gp.CHUNK_TILES]:
        passes = gp.chunks(total, k)
        assert len(passes) >= 2 and sum(p[1] for p in passes) == total
        nbytes, got = gp.workspace_bytes(name, mode, k), []
        for rep in range(2):
            ws = Guarded('workspace of %d tiles of tape' % k, nbytes, FILL, dev)
            grad = Guarded('dparams, %d tiles of tape' % k, eng.nparams * 4, FILL, dev)
            rc = lib.bhn_render_bwd(M, m, su['packed'].ptr, C.byref(gs), C.byref(fs), ptr(su['dimg']), grad.ptr, ws.ptr, nbytes, st)
            torch.cuda.synchronize()
            assert rc == 0, (name, k, lib.bhn_last_error())
            assert not ws.disturbed() and not grad.disturbed(), (name, k, ws.disturbed(), grad.disturbed())
            got.append(grad.f32().copy())
        assert np.isfinite(got[0]).all(), (name, mode, k, 'not finite')
        d = first_difference(got[1], got[0])
        assert d is None, 'case %r %s, %d tiles of tape: the second run differs, first at element %d (%r vs %r)' % ((name, mode, k) + d)
        worst = 0.0
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            x, y = got[0][c0:c1].astype(np.float64), full[c0:c1].astype(np.float64)
            worst = max(worst, float((np.abs(x - y) / (1e-6 * np.abs(y).max() + 1e-5 * np.abs(y))).max()))
        print('\n[general path] %-32s %-4s %2d tiles of tape: %2d passes (last %d tiles, %d cut a frame)  vs all at once %.3f of the bound'
              % (name, mode, k, len(passes), passes[-1][1], sum(1 for p in passes if gp.cuts_a_frame(p, L['tiles_per_frame'])), worst))
        assert worst <= 1.0, 'case %r %s, %d tiles of tape: %.3g of the bound against the all-at-once gradient' % (name, mode, k, worst)
