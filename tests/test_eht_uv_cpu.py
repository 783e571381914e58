"""CPU tests of the matrix-free EHT losses (libbhnerf_eht.so, csrc/eht_uv.hip, observation.DirectDFT): everything about them
that needs no device.

The plan (workspace layout, row splits) and the per-element arithmetic live in csrc/eht_uv.h and compile with a plain C++
compiler.  tools/eht_uv_host.cpp walks the launches of bhn_eht_vis / bhn_eht_chi2_uv one workgroup after the other; here it is
built with g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process with its outputs and workspace in heap blocks of exactly
the documented sizes, and compared with the float64 table-form reference of tests/eht_uv_cases.py at the project's f32 bound
(2e-5 of the largest element; the loss 2e-5 relative).  Nothing built with a sanitizer is loaded into this Python process.

Also here: DirectDFT.dense() against observation.dft_matrix, closure_table, the batching of TemporalBatchedArgs, the float64
reference itself against oracle_np.loss_eht on the dense conjugated-legs form, and the symbol table of the library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import observation                                     # noqa: E402

DTYPES = ('vis', 'amp', 'cphase')


def test_dense_equals_dft_matrix_bitwise_and_is_row_major():
    rng = np.random.default_rng(3)
    uv = rng.normal(size=(3, 6, 2)) * 3e9
    for npix in (8, 13):
        want = np.stack([observation.dft_matrix(u, E.FOV, npix) for u in uv])
        got = observation.DirectDFT(uv, E.FOV, npix).dense()
        assert got.dtype == np.complex64 and got.tobytes() == want.tobytes()
    for name in E.CASES:
        c = E.case(name)
        got = E.operator(c, 'vis').dense(np.complex128)
        assert got.shape == (c['B'], len(c['pairs']), c['H'] * c['W'])
        assert np.abs(got - c['A128']).max() < 1e-12                  # H rows of W pixels: x runs fastest
        # the transposed convention (W rows of H pixels) is a different matrix
        assert np.abs(got - E.dense128(c['uv'], E.FOV, c['W'], c['H'])).max() > 0.1
        # pixel (y, x) alone: the phase is -2 pi (u x_x + v y_y)
        y, x, k = 2, 5, 1
        xx, yy = (x - (c['W'] - 1) / 2.0) * E.FOV / c['W'], (y - (c['H'] - 1) / 2.0) * E.FOV / c['H']
        want = np.exp(-2j * np.pi * (c['uv'][0, k, 0] * xx + c['uv'][0, k, 1] * yy))
        assert abs(got[0, k, y * c['W'] + x] - want) < 1e-9


def test_dense_with_triangles_is_the_conjugated_legs_form():
    c = E.case('12x20')
    A = E.operator(c, 'vis').dense()
    pairs = {tuple(p): i for i, p in enumerate(c['pairs'].tolist())}
    idx = np.array([[pairs[(a, b)], pairs[(b, d)], pairs[(a, d)]] for a, b, d in c['triangles']])      # test_gpu_eht2017.py's table
    A3 = np.stack([A[:, idx[:, k]] for k in range(3)], axis=1)
    A3[:, 2] = np.conj(A3[:, 2])
    got = E.operator(c, 'cphase').dense()
    assert got.shape == (c['B'], 3, 10, c['H'] * c['W']) and got.tobytes() == A3.tobytes()


def test_closure_table():
    c = E.case('12x20')
    pairs = {tuple(p): i for i, p in enumerate(c['pairs'].tolist())}
    idx = np.array([[pairs[(a, b)], pairs[(b, d)], pairs[(a, d)]] for a, b, d in c['triangles']])
    assert c['tri'].dtype == np.int32 and c['sign'].dtype == np.int8
    assert np.array_equal(c['tri'], idx) and np.array_equal(c['sign'], np.tile(np.array([1, 1, -1], dtype=np.int8), (10, 1)))
    # a baseline stored the other way round serves the same legs with the opposite sign
    rev = c['pairs'].copy()
    rev[3] = rev[3][::-1]
    tri, sign = observation.closure_table(rev, c['triangles'])
    assert np.array_equal(tri, idx)
    flipped = (idx == 3)
    assert flipped.sum() == 3 and np.array_equal(sign[flipped], -c['sign'][flipped]) and np.array_equal(sign[~flipped], c['sign'][~flipped])
    with pytest.raises(ValueError, match='baseline'):
        observation.closure_table(np.delete(c['pairs'], 3, axis=0), c['triangles'])
    with pytest.raises(AttributeError):                                # an index outside the baselines
        observation.DirectDFT(c['uv'], E.FOV, 8, triangles=(np.array([[0, 1, 10]]), np.array([[1, 1, -1]])))


def test_temporal_batched_args_keeps_the_operator_and_its_float64_uv():
    from bhnerf_amd import optimization, units
    c = E.case('12x20')
    op = E.operator(c, 'cphase')
    t_frames = np.arange(c['B']) * 0.1 * units.hr
    target = np.arange(c['B'] * 10, dtype=np.float64).reshape(c['B'], 10)
    args = optimization.TemporalBatchedArgs(t_frames, [target, np.ones_like(target), op])
    import torch
    key = [2, 0]
    tgt, sig, got, t = args[key]
    assert isinstance(got, observation.DirectDFT) and got.shape == (2, 10, 2) and (got.H, got.W) == (12, 20) and got.ncp == 10
    uv = got.uv.cpu().numpy() if isinstance(got.uv, torch.Tensor) else got.uv
    assert uv.dtype == np.float64 and uv.tobytes() == c['uv'][key].tobytes()             # not rounded through float32
    want = op.take(key)
    assert np.array_equal(np.asarray(want.uv), c['uv'][key]) and want.uv.dtype == np.float64
    assert not isinstance(tgt, observation.DirectDFT) and np.array_equal(np.asarray(tgt.cpu() if hasattr(tgt, 'cpu') else tgt), target[key].astype(np.float32))
    assert np.array_equal(t, np.asarray(units.strip(t_frames))[key])
    # arrays are batched as before
    dense = optimization.TemporalBatchedArgs(t_frames, [target, op.dense()])[key]
    assert tuple(dense[1].shape) == (2, 3, 10, 240) and not isinstance(dense[1], observation.DirectDFT)
    step = optimization.TrainStep.eht_uv(t_frames, target, np.ones_like(target), c['uv'], E.FOV, (12, 20), dtype='cphase',
                                         triangles=c['triangles'], pairs=c['pairs'])
    assert isinstance(step.args[0].host_args[2], observation.DirectDFT) and step.args[0].host_args[2].uv.dtype == np.float64
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_uv(t_frames, target, np.ones_like(target), c['uv'], E.FOV, (12, 20), dtype='cphase')
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_uv(t_frames, target, np.ones_like(target), c['uv'], E.FOV, (12, 20), dtype='vis',
                                      triangles=c['triangles'], pairs=c['pairs'])


@pytest.mark.parametrize('name', list(E.CASES))
def test_table_form_reference_equals_the_dense_oracle(name):
    from oracle import oracle_np as onp
    c = E.case(name)
    assert c['min_amp'] >= E.MIN_AMP, c['min_amp']
    print('\n[eht uv] %s: smallest |vis| / largest = %.3f' % (name, c['min_amp']))
    img64 = c['images'].astype(np.float64)
    for dtype in DTYPES:
        A = E.operator(c, dtype).dense(np.complex128)
        target, sigma = c['data'][dtype]
        t64 = target.astype(np.complex128 if dtype == 'vis' else np.float64)
        loss, grad, _ = c['ref'][dtype]
        want = onp.loss_eht(img64, t64, sigma.astype(np.float64), A, 1.0, dtype)
        assert abs(loss - want) <= 1e-9 * abs(want), (dtype, loss, want)
        ref_loss, ref_grad = E.dense_ref_loss(img64, A, t64, sigma.astype(np.float64), 1.0, dtype)
        assert abs(ref_loss - want) <= 1e-9 * abs(want)
        assert E.rel_max(grad, ref_grad) < 1e-9, dtype


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/eht_uv_host.cpp built with the sanitizers -> run(case dict, dtype, want_grad) -> (vis, loss, dimages or None)."""
    exe, work = side.build_host_program(tmp_path_factory, 'eht_uv_host')

    def run(c, dtype, want_grad=True, scale=1.0, tag='case'):
        H, W, B, Sx = c['H'], c['W'], c['B'], max(c['Sx'], 1)
        N, nvis = B * Sx, len(c['pairs'])
        ncp = len(c['tri']) if dtype == 'cphase' else 0
        target, sigma = c['data'][dtype]
        psize_y, psize_x = E.FOV / H, E.FOV / W
        head = np.array([N, Sx, nvis, ncp, H, W, DTYPES.index(dtype), int(want_grad), psize_x, psize_y, scale], dtype=np.float64)
        tgt = np.ascontiguousarray(target).view(np.float32) if dtype == 'vis' else target.astype(np.float32)
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        with open(fin, 'wb') as f:
            for a in (head, c['uv'], c['images'], tgt, sigma.astype(np.float32)) + ((c['tri'], c['sign']) if ncp else ()):
                f.write(np.ascontiguousarray(a).tobytes())
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        npix = N * H * W
        assert len(raw) == 8 * N * nvis + 4 + (4 * npix if want_grad else 0)          # the documented sizes, nothing else
        vis = np.frombuffer(raw, dtype=np.complex64, count=N * nvis).reshape(target.shape[:-1] + (nvis,))
        loss = float(np.frombuffer(raw, dtype=np.float32, count=1, offset=8 * N * nvis)[0])
        dimg = np.frombuffer(raw, dtype=np.float32, count=npix, offset=8 * N * nvis + 4).reshape(c['images'].shape) if want_grad else None
        return vis, loss, dimg
    return run


@pytest.mark.parametrize('name,Sx', [('12x20', 0), ('13x7', 0), ('12x20', 2)])
def test_host_build_of_the_plan_and_arithmetic_meets_the_float64_reference(host_program, name, Sx):
    c = E.case(name, Sx)
    assert c['min_amp'] >= E.MIN_AMP
    for dtype in DTYPES:
        ref_loss, ref_grad, ref_vis = c['ref'][dtype]
        vis, loss, dimg = host_program(c, dtype, tag='%s_%d_%s' % (name, Sx, dtype))
        assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss)       # every element written
        e_vis, e_loss, e_grad = E.rel_max(vis, ref_vis), abs(loss - ref_loss) / abs(ref_loss), E.rel_max(dimg, ref_grad)
        print('\n[eht uv, host build] %s Sx %d %-6s vis %.1e loss %.1e dimages %.1e' % (name, Sx, dtype, e_vis, e_loss, e_grad))
        assert e_vis <= E.F32_TOL and e_loss <= E.F32_TOL and e_grad <= E.F32_TOL, (dtype, e_vis, e_loss, e_grad)
        # forward only, and the loss scale
        vis0, loss0, none = host_program(c, dtype, want_grad=False, tag='nograd')
        assert none is None and loss0 == loss and vis0.tobytes() == vis.tobytes()
        _, loss2, dimg2 = host_program(c, dtype, scale=2.0, tag='scale2')
        assert abs(loss2 - 2 * loss) <= 1e-6 * abs(loss2) and np.abs(dimg2 - 2 * dimg).max() <= 1e-6 * np.abs(dimg2).max()


def test_host_build_zero_gradient_at_zero_visibility(host_program):
    """An all-zero image has |vis| = 0 on every baseline: the 'amp' and 'cphase' gradients are zero there, not NaN."""
    c = dict(E.case('13x7'))
    c['images'] = np.zeros_like(c['images'])
    for dtype in ('amp', 'cphase'):
        vis, loss, dimg = host_program(c, dtype, tag='zero_' + dtype)
        assert not vis.any() and np.isfinite(loss) and not dimg.any()


def test_plan_row_splits_cover_every_row_once(host_program):
    """Shapes at which the split arithmetic takes its other paths: one row, fewer rows than a split holds, a remainder, more
    than one 256-column trip, nvis below and above a baseline block.  The host program's visibilities must equal A . image."""
    rng = np.random.default_rng(7)
    for H, W, ns in ((1, 5, 3), (7, 300, 3), (9, 3, 6), (70, 9, 5), (130, 2, 3)):
        pos = rng.normal(size=(1, ns, 2)) * 3e9
        pairs = np.array([(i, j) for i in range(ns) for j in range(i + 1, ns)])
        uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])
        images = E.blobs(rng, (1, H, W))
        A = E.dense128(uv, E.FOV, H, W)
        target = np.zeros((1, len(pairs)), dtype=np.complex64)
        ref_loss, ref_grad, ref_vis = E.table_loss(images, A, target, np.ones((1, len(pairs))), 1.0, 'vis')
        c = dict(H=H, W=W, B=1, Sx=0, pairs=pairs, uv=uv, images=images, tri=None, sign=None,
                 data={'vis': (target, np.ones((1, len(pairs)), dtype=np.float32))})
        vis, loss, dimg = host_program(c, 'vis', tag='split')
        assert E.rel_max(vis, ref_vis) <= E.F32_TOL and abs(loss - ref_loss) <= E.F32_TOL * ref_loss and E.rel_max(dimg, ref_grad) <= E.F32_TOL, (H, W, ns)


def test_observe_without_a_device_raises_the_package_error(monkeypatch):
    import torch
    from bhnerf_amd import _hip
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    c = E.case('13x7')
    with pytest.raises(_hip.HipError):
        E.operator(c, 'vis').observe(c['images'])


def test_argument_validation_returns_before_any_device_call():
    import ctypes as C
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.eht_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    N, Sx, nvis, ncp, H, W = 4, 2, 10, 10, 12, 20
    need = lib.bhn_eht_ws_bytes(N, nvis, ncp, H, W)
    assert need > 0 and need % 256 == 0 and lib.bhn_eht_ws_bytes(N, nvis, 0, H, W) <= need
    for bad in ((0, nvis, ncp, H, W), (N, 0, ncp, H, W), (N, nvis, -1, H, W), (N, nvis, ncp, 0, W), (N, nvis, ncp, H, 0)):
        assert lib.bhn_eht_ws_bytes(*bad) == 0
    good = dict(images=p, uv=p, N=N, Sx=Sx, nvis=nvis, H=H, W=W, psize_x=1e-11, psize_y=1e-11, dtype=2, target=p, sigma=p, scale=1.0,
                tri=p, tri_sign=p, ncp=ncp, loss=p, dimages=p, ws=p, ws_bytes=need)
    order = list(good)
    bad = [(dict(images=None), b'null', 1), (dict(uv=None), b'null', 1), (dict(target=None), b'null', 1), (dict(sigma=None), b'null', 1),
           (dict(loss=None), b'null', 1), (dict(ws=None), b'null', 1), (dict(N=0), b'sizes below 1', 1), (dict(nvis=0), b'sizes below 1', 1),
           (dict(H=0), b'sizes below 1', 1), (dict(W=-2), b'sizes below 1', 1), (dict(Sx=0), b'sizes below 1', 1), (dict(Sx=3), b'multiple of Sx', 1),
           (dict(psize_x=0.0), b'pixel sizes', 1), (dict(psize_y=float('nan')), b'pixel sizes', 1), (dict(dtype=3), b'not supported', 1),
           (dict(tri=None), b'NULL table', 1), (dict(tri_sign=None), b'NULL table', 1), (dict(ncp=0), b'need a triangle table', 1),
           (dict(ncp=-1), b'need a triangle table', 1), (dict(ws=C.c_void_p(4100)), b'aligned', 1),
           (dict(ws_bytes=need - 1), b'workspace of', _hip.BHN_EWORKSPACE)]
    for change, word, code in bad:
        a = dict(good, **change)
        rc = lib.bhn_eht_chi2_uv(*[a[k] for k in order], None)
        assert rc == code, (change, rc)
        msg = lib.bhn_eht_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_eht'):
            _hip.eht_check(rc)
    vgood = dict(images=p, uv=p, N=N, Sx=Sx, nvis=nvis, H=H, W=W, psize_x=1e-11, psize_y=1e-11, vis_out=p, ws=p,
                 ws_bytes=lib.bhn_eht_ws_bytes(N, nvis, 0, H, W))
    for change, code in ((dict(vis_out=None), 1), (dict(images=None), 1), (dict(N=0), 1), (dict(vis_out=C.c_void_p(4100)), 1),
                         (dict(ws_bytes=vgood['ws_bytes'] - 1), _hip.BHN_EWORKSPACE)):
        a = dict(vgood, **change)
        assert lib.bhn_eht_vis(*[a[k] for k in vgood], None) == code, change


def test_eht_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_eht.so: the dynamic symbol table is the declarations of include/bhnerf_eht.h and nothing else, the ctypes table
    binds exactly those, and the library references no allocator, no getenv and no synchronisation.  The other two libraries and
    include/bhnerf_hip.h know nothing of it."""
    from bhnerf_amd import _hip
    side.assert_library_conventions('bhnerf_eht.h', _hip.EHT_LIB_PATH, _hip.EHT_SIGNATURES, 'bhn_eht',
                                    ['bhn_eht_chi2_uv', 'bhn_eht_last_error', 'bhn_eht_vis', 'bhn_eht_ws_bytes'])
