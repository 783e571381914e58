"""GPU tests of the (u, v) EHT kernels at the edge shapes of tests/eht_edge_cases.py: more than one wave in the forward sum, more
than one column trip, adjoint column blocks past the first, more than 256 baselines / triangles / quadrangles per plane, more than
256 planes, the row-split cap and a short last split, thousands of whole turns in the twiddle phase, one pixel.  Every case runs
through libbhnerf_eht.so (observe and 'vis' | 'amp' | 'cphase', with and without gradient); the cases that reach their own kernels
run through libbhnerf_cls.so ('amp+cphase+logcamp') and libbhnerf_pol.so ('pvis+m', Sx 3 and 4), which compile the same forward
and adjoint text into objects of their own.  Against the float64 references of the table, at each family's existing bound
(eht_uv_cases.F32_TOL, test_gpu_closure.LOGCAMP_BOUND, pol_cases.M_BOUND); tests/test_eht_edge_cases_cpu.py proves that these
bounds see the slips each case is for.  Worst figures measured on an MI355X: DESIGN 4.10, 'edge shapes'."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closure_cases as K                                              # noqa: E402
import eht_edge_cases as T                                             # noqa: E402
import eht_uv_cases as E                                               # noqa: E402
import pol_cases as P                                                  # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401

UV_DTYPES = ('vis', 'amp', 'cphase')
GUARD = 4096          # bytes on either side of a buffer: 0xA5 there, the buffer itself poisoned with NaN bytes (0xFF)
a256 = lambda v: (v + 255) // 256 * 256


def _uv_chi2(d, dtype, dev, want_grad=True, op=None, images=None, data=None):
    from bhnerf_amd import engine
    target, sigma = data if data is not None else d['data'][dtype]
    images = torch.as_tensor(d['images'] if images is None else images, device=dev)
    return engine.chi2_eht(images, op if op is not None else E.operator(d, dtype), target, sigma, 1.0, dtype, want_grad=want_grad)


def _cls_chi2(d, dev, want_grad=True, op=None, images=None, data=None):
    from bhnerf_amd import engine
    op = op if op is not None else K.operator(d, T.CLS_DTYPE, K.WEIGHTS)
    target, sigma = data if data is not None else K.packed(d, T.CLS_DTYPE)
    images = torch.as_tensor(d['images'] if images is None else images, device=dev)
    loss, dimg = engine.chi2_eht(images, op, target, sigma, T.CLS_SCALE, T.CLS_DTYPE, want_grad=want_grad)
    return loss, dimg, op.last_terms.cpu().numpy()


def _pol_chi2(d, dev, want_grad=True, op=None, images=None, data=None):
    from bhnerf_amd import engine
    op = op if op is not None else P.operator(d, P.WEIGHTS)
    target, sigma = data if data is not None else P.packed(d, T.POL_DTYPE)
    images = torch.as_tensor(d['images'] if images is None else images, device=dev)
    loss, dimg = engine.chi2_eht(images, op, target, sigma, P.SCALE, T.POL_DTYPE, want_grad=want_grad)
    return loss, dimg, op.last_terms.cpu().numpy()


@pytest.mark.parametrize('name,Sx', T.UV_PARAMS)
def test_uv_library_meets_float64(dev, name, Sx):
    c, d = T.BY_NAME[name], T.uv(name, Sx)
    T.admitted(name)
    vis = E.operator(d, 'vis').observe(d['images'])
    ref_vis = d['ref']['vis'][2]
    assert vis.is_cuda and vis.dtype == torch.complex64 and tuple(vis.shape) == ref_vis.shape
    worst = {'vis': E.rel_max(vis.cpu().numpy(), ref_vis)}
    assert worst['vis'] <= E.F32_TOL, worst
    if name == 'one':                                                  # the twiddles at the centre pixel are (1, 0)
        got = vis.cpu().numpy()
        assert np.array_equal(got.real, np.full(got.shape, d['images'][0, 0, 0])) and not got.imag.any()
    for dtype in c.uv:
        ref_loss, ref_grad, _ = T.uv_reference(name, Sx, dtype)
        for want_grad in (True, False):
            loss, dimg = _uv_chi2(d, dtype, dev, want_grad)
            e_loss = T.rel_loss(loss.item(), ref_loss)
            worst[dtype + ' loss'] = max(worst.get(dtype + ' loss', 0.0), e_loss)
            assert e_loss <= T.uv_bound(dtype, 'loss'), (dtype, want_grad, loss.item(), ref_loss)
            if not want_grad:
                assert dimg is None
                continue
            assert dimg.shape == d['images'].shape and dimg.dtype == torch.float32
            worst[dtype + ' dimages'] = T.rel_max(dimg.cpu().numpy(), ref_grad)
            assert worst[dtype + ' dimages'] <= T.uv_bound(dtype, 'dimages'), (dtype, worst)
    print('\n[eht edges] uv  %-8s Sx %d  %s' % (name, Sx, '  '.join('%s %.1e' % kv for kv in worst.items())))


@pytest.mark.parametrize('name,Sx', T.CLS_PARAMS)
def test_closure_library_meets_float64(dev, name, Sx):
    d, terms = T.cls(name, Sx), T.CLS_DTYPE.split('+')
    T.admitted(name)
    ref = T.cls_reference(name, Sx)
    for want_grad in (True, False):
        loss, dimg, four = _cls_chi2(d, dev, want_grad)
        assert loss.item() == four[0] and (dimg is None) == (not want_grad)
        parts = {t: float(four[1 + K.TERMS.index(t)]) for t in terms}
        err = K.errors(T.CLS_DTYPE, loss.item(), parts, dimg.cpu().numpy() if want_grad else None, ref)
        print('\n[eht edges] cls %-8s Sx %d  %s' % (name, Sx, '  '.join('%s %.1e' % kv for kv in err.items())), end='')
        for t in terms:
            assert err[t] <= T.cls_bound([t], 'loss'), (t, err)
        assert err['total'] <= T.cls_bound(terms, 'loss'), err
        if want_grad:
            assert dimg.shape == d['images'].shape and err['dimages'] <= T.cls_bound(terms, 'dimages'), err
    print()


@pytest.mark.parametrize('name,Sx', T.POL_PARAMS)
def test_pol_library_meets_float64(dev, name, Sx):
    d, terms = T.pol(name, Sx), T.POL_DTYPE.split('+')
    ref = T.pol_reference(name, Sx)
    for want_grad in (True, False):
        loss, dimg, three = _pol_chi2(d, dev, want_grad)
        assert loss.item() == three[0] and (dimg is None) == (not want_grad)
        parts = {t: float(three[1 + P.TERMS.index(t)]) for t in terms}
        err = P.errors(T.POL_DTYPE, loss.item(), parts, dimg.cpu().numpy() if want_grad else None, ref)
        print('\n[eht edges] pol %-8s Sx %d  %s' % (name, Sx, '  '.join('%s %.1e' % kv for kv in err.items())), end='')
        for t in terms:
            assert err[t] <= T.pol_bound([t], 'loss'), (t, err)
        assert err['total'] <= T.pol_bound(terms, 'loss'), err
        if want_grad:
            assert dimg.shape == d['images'].shape and (Sx == 3 or not bool(dimg[:, 3].any()))             # the V plane: zeros
            assert err['dimages'] <= T.pol_bound(terms, 'dimages'), err
    print()


def test_w300_is_bitwise_reproducible_and_independent_of_the_batch(dev):
    """Two column trips, two adjoint column blocks, B = 2: two calls give equal bytes, and frame 1 alone (B = 1) is row 1 of the
    B = 2 call, in each library."""
    d = T.uv('w300')
    for dtype in UV_DTYPES:
        op = E.operator(d, dtype)
        loss, dimg = _uv_chi2(d, dtype, dev, op=op)
        loss2, dimg2 = _uv_chi2(d, dtype, dev, op=op)
        assert torch.equal(loss, loss2) and torch.equal(dimg, dimg2)
        vis = op.observe(d['images'])
        assert torch.equal(torch.view_as_real(vis), torch.view_as_real(op.observe(d['images'])))
        tg, sg = d['data'][dtype]
        op1 = op.take([1])
        _, dimg1 = _uv_chi2(d, dtype, dev, op=op1, images=d['images'][1:2], data=(tg[1:2], sg[1:2]))
        assert torch.equal(dimg1[0], dimg[1])
        assert torch.equal(torch.view_as_real(op1.observe(d['images'][1:2]))[0], torch.view_as_real(vis)[1])
    for lib, d, chi2, packed in (('cls', T.cls('w300'), _cls_chi2, lambda d: K.packed(d, T.CLS_DTYPE)),
                                 ('pol', T.pol('w300', 3), _pol_chi2, lambda d: P.packed(d, T.POL_DTYPE))):
        op = K.operator(d, T.CLS_DTYPE, K.WEIGHTS) if lib == 'cls' else P.operator(d, P.WEIGHTS)
        loss, dimg, terms = chi2(d, dev, op=op)
        loss2, dimg2, terms2 = chi2(d, dev, op=op)
        assert torch.equal(loss, loss2) and torch.equal(dimg, dimg2) and terms.tobytes() == terms2.tobytes(), lib
        assert chi2(d, dev, want_grad=False, op=op)[2].tobytes() == terms.tobytes(), lib                     # forward only: the same floats
        tg, sg = packed(d)
        _, dimg1, _ = chi2(d, dev, op=op.take([1]), images=d['images'][1:2], data=(tg[1:2], sg[1:2]))
        assert torch.equal(dimg1[0], dimg[1]), lib


def _contract(dev, label, call, need, N, npix, nloss, check):
    """The caller-owned-buffer contract on poisoned buffers of exactly the documented sizes between guard bands: one byte too
    little workspace is refused and nothing is launched; forward only leaves dimages alone; with the gradient every element of
    every output is written and no guard byte is disturbed.  check(loss float32[nloss], dimages or None, ws bytes)."""
    from bhnerf_amd import _hip
    mk = lambda what, nbytes: Guarded('%s %s' % (label, what), nbytes, 0xFF, dev, guard=GUARD, guard_fill=0xA5)
    loss, dimg, ws = mk('loss', 4 * nloss), mk('dimages', 4 * npix), mk('ws', need)
    intact = lambda: all(b.disturbed() is None for b in (loss, dimg, ws))
    assert call(loss.ptr, dimg.ptr, ws.ptr, need - 1) == _hip.BHN_EWORKSPACE
    torch.cuda.synchronize()
    assert loss.untouched() and dimg.untouched() and ws.untouched()
    assert call(loss.ptr, None, ws.ptr, need) == 0
    torch.cuda.synchronize()
    assert dimg.untouched() and np.isfinite(loss.f32()).all() and intact()
    forward_only = loss.f32().copy()
    check(forward_only, None, None)
    loss.mid.fill_(0xFF); ws.mid.fill_(0xFF)
    assert call(loss.ptr, dimg.ptr, ws.ptr, need) == 0
    torch.cuda.synchronize()
    assert intact(), [b.disturbed() for b in (loss, dimg, ws)]
    got = dimg.f32()
    assert dimg.poisoned(4) == 0 and np.isfinite(got).all() and np.isfinite(loss.f32()).all()              # every element written
    assert loss.f32().tobytes() == forward_only.tobytes()
    check(loss.f32(), got, ws.mid)


def _uv_vis(d, dev):
    """bhn_eht_vis on the images of a case dict: (B, [Sx,] nvis, 2) float32 on the device."""
    from bhnerf_amd import engine, observation
    op = observation.DirectDFT(d['uv'], E.FOV, (d['H'], d['W'])).to(dev)
    return torch.view_as_real(engine.eht_vis_uv(torch.as_tensor(d['images'], device=dev), op))


@pytest.mark.parametrize('name', T.CONTRACT)
def test_uv_buffer_contract(dev, name):
    from bhnerf_amd import _hip
    lib = _hip.eht_lib()
    d = T.uv(name)
    H, W, N, nvis = d['H'], d['W'], d['B'], len(d['pairs'])
    img, uv = torch.as_tensor(d['images'], device=dev).contiguous(), torch.as_tensor(d['uv'], device=dev)
    tri, sign = torch.as_tensor(d['tri'], device=dev), torch.as_tensor(d['sign'], device=dev)
    psx, psy, stream = E.FOV / W, E.FOV / H, _hip.stream_ptr(dev)
    for dtype in UV_DTYPES:
        ncp = len(d['tri']) if dtype == 'cphase' else 0
        target, sigma = d['data'][dtype]
        tgt = torch.as_tensor(np.ascontiguousarray(target).view(np.float32) if dtype == 'vis' else target, device=dev).contiguous()
        sig = torch.as_tensor(sigma, device=dev).contiguous()
        need = int(lib.bhn_eht_ws_bytes(N, nvis, ncp, H, W))
        assert need > 0
        ref_loss, ref_grad, _ = T.uv_reference(name, 0, dtype)

        def call(loss, dimages, ws, ws_bytes):
            return lib.bhn_eht_chi2_uv(_hip.ptr(img), _hip.ptr(uv), N, 1, nvis, H, W, psx, psy, UV_DTYPES.index(dtype), _hip.ptr(tgt), _hip.ptr(sig),
                                       1.0, _hip.ptr(tri) if ncp else None, _hip.ptr(sign) if ncp else None, ncp, loss, dimages, ws, ws_bytes, stream)

        def check(loss, got, ws):
            assert T.rel_loss(float(loss[0]), ref_loss) <= T.uv_bound(dtype, 'loss')
            assert got is None or E.rel_max(got.reshape(ref_grad.shape), ref_grad) <= T.uv_bound(dtype, 'dimages')
        _contract(dev, 'uv %s %s' % (name, dtype), call, need, N, N * H * W, 1, check)
    # bhn_eht_vis, the same way
    need = int(lib.bhn_eht_ws_bytes(N, nvis, 0, H, W))
    vis, ws = (Guarded(what, n, 0xFF, dev, guard=GUARD, guard_fill=0xA5) for what, n in (('vis', 8 * N * nvis), ('ws of bhn_eht_vis', need)))
    args = (_hip.ptr(img), _hip.ptr(uv), N, 1, nvis, H, W, psx, psy, vis.ptr, ws.ptr)
    assert lib.bhn_eht_vis(*args, need - 1, stream) == _hip.BHN_EWORKSPACE
    torch.cuda.synchronize()
    assert vis.untouched() and ws.untouched()
    assert lib.bhn_eht_vis(*args, need, stream) == 0
    torch.cuda.synchronize()
    assert vis.disturbed() is None and ws.disturbed() is None and vis.poisoned(4) == 0
    got = vis.f32().view(np.complex64).reshape(d['ref']['vis'][2].shape)
    assert np.isfinite(got.view(np.float32)).all() and E.rel_max(got, d['ref']['vis'][2]) <= E.F32_TOL


@pytest.mark.parametrize('name', T.CONTRACT)
def test_closure_buffer_contract_and_workspace_visibilities(dev, name):
    from bhnerf_amd import _hip
    lib = _hip.cls_lib()
    d, terms = T.cls(name), T.CLS_DTYPE.split('+')
    H, W, N, nvis, ncp, nca = d['H'], d['W'], d['B'], len(d['pairs']), len(d['tri']), len(d['quad'])
    img, uv = torch.as_tensor(d['images'], device=dev).contiguous(), torch.as_tensor(d['uv'], device=dev)
    held = {t: [torch.as_tensor(a, device=dev).contiguous() for a in d['data'][t]] for t in terms}
    structs = {t: _hip.bhn_cls_term(v[0].data_ptr(), v[1].data_ptr(), K.WEIGHTS[t]) for t, v in held.items()}
    tri, sign, quad = (torch.as_tensor(d[k], device=dev) for k in ('tri', 'sign', 'quad'))
    need = int(lib.bhn_cls_ws_bytes(N, nvis, ncp, nca, H, W))
    assert need > 0
    ref_total, ref_grad, ref_parts, _ = T.cls_reference(name, 0)
    want_vis = _uv_vis(d, dev)

    def call(loss, dimages, ws, ws_bytes):
        return lib.bhn_cls_chi2(_hip.ptr(img), _hip.ptr(uv), N, 1, nvis, H, W, E.FOV / W, E.FOV / H, C.byref(structs['amp']), C.byref(structs['cphase']),
                                C.byref(structs['logcamp']), _hip.ptr(tri), _hip.ptr(sign), ncp, _hip.ptr(quad), nca, T.CLS_SCALE, loss, dimages, ws,
                                ws_bytes, _hip.stream_ptr(dev))

    def check(four, got, ws):
        assert abs(float(four[0]) - ref_total) <= T.cls_bound(terms, 'loss') * abs(ref_total)
        for t in terms:
            assert abs(float(four[1 + K.TERMS.index(t)]) - ref_parts[t]) <= T.cls_bound([t], 'loss') * abs(ref_parts[t]), t
        if got is None:
            return
        assert E.rel_max(got.reshape(ref_grad.shape), ref_grad) <= T.cls_bound(terms, 'dimages')
        # V sits where the (u, v) library's plan puts it (..., V, dphi, loss slots), and is bhn_eht_vis' bit for bit
        eht_bytes = int(_hip.eht_lib().bhn_eht_ws_bytes(N, nvis, ncp, H, W))
        off_vis = eht_bytes - a256(4 * N) - a256(4 * N * ncp) - a256(8 * N * nvis)
        assert torch.equal(ws[off_vis:off_vis + 8 * N * nvis].view(torch.float32).reshape(want_vis.shape), want_vis)
    _contract(dev, 'cls %s' % name, call, need, N, N * H * W, 4, check)


@pytest.mark.parametrize('name', T.CONTRACT)
def test_pol_buffer_contract_and_workspace_visibilities(dev, name):
    from bhnerf_amd import _hip
    from test_gpu_pol import _raw
    d, terms = T.pol(name, 3), T.POL_DTYPE.split('+')
    r = _raw(d, dev)                                                    # (its terms carry weight 1)
    N, nvis, H, W = r['N'], r['nvis'], d['H'], d['W']
    ref_total, ref_grad, ref_parts, _ = P.pol_loss(d['images'], d['A128'], d['data'], terms, {t: 1.0 for t in terms}, 1.0)
    want_vis = _uv_vis(d, dev)

    def check(three, got, ws):
        assert abs(float(three[0]) - ref_total) <= T.pol_bound(terms, 'loss') * abs(ref_total)
        for t in terms:
            assert abs(float(three[1 + P.TERMS.index(t)]) - ref_parts[t]) <= T.pol_bound([t], 'loss') * abs(ref_parts[t]), t
        if got is None:
            return
        assert E.rel_max(got.reshape(ref_grad.shape), ref_grad) <= T.pol_bound(terms, 'dimages')
        eht_bytes = int(_hip.eht_lib().bhn_eht_ws_bytes(N, nvis, 0, H, W))
        off_vis = eht_bytes - a256(4 * N) - a256(8 * N * nvis)                                # EhtPlan: ..., V, dphi (none), loss slots
        assert torch.equal(ws[off_vis:off_vis + 8 * N * nvis].view(torch.float32).reshape(want_vis.shape), want_vis)
    _contract(dev, 'pol %s' % name, lambda loss, dimages, ws, ws_bytes: r['call'](terms, loss, dimages, ws, ws_bytes), r['need'], N, N * H * W, 3, check)
