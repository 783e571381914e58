"""CPU tests of the combined closure loss (libbhnerf_cls.so, csrc/eht_closure.hip, observation.ClosureDFT): everything about it
that needs no device.

The plan and the arithmetic of the new term live in csrc/eht_closure.h on top of csrc/eht_uv.h and compile with a plain C++
compiler.  tools/eht_closure_host.cpp walks the launches of bhn_cls_chi2 one workgroup after the other; here it is built with
g++ -O2 and the sanitizers (tests/side_lib_support.py), run as a child process with its outputs and workspace in heap blocks of
exactly the documented sizes, and compared with the float64 reference of tests/closure_cases.py.  Nothing built with a sanitizer
is loaded into this Python process.

Bounds.  The 'amp' and 'cphase' terms, and totals and gradients made of them alone, are held to the project's f32 bound
(eht_uv_cases.F32_TOL: the loss relative, dimages relative to its largest element).  The 'logcamp' term divides by |V| four times
and its residual over sigma is of order 10; it and every total or gradient that contains it are held to LOGCAMP_BOUND = 1e-3, the
ceiling that the measured bounds of tests/test_gpu_closure.py may never exceed.  The figures are printed."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closure_cases as K                                              # noqa: E402
import eht_uv_cases as E                                               # noqa: E402
import side_lib_support as side                                        # noqa: E402
from bhnerf_amd import observation                                     # noqa: E402

LOGCAMP_BOUND = 1e-3


def bound(names):
    """The bound of a figure made of the terms `names`."""
    return LOGCAMP_BOUND if 'logcamp' in names else E.F32_TOL


def test_closure_quadrangles_and_the_quadrangle_table():
    assert observation.closure_quadrangles(3).shape == (0, 4, 2)
    q4 = observation.closure_quadrangles(4)
    assert q4.tolist() == [[[0, 1], [2, 3], [0, 2], [1, 3]], [[0, 3], [1, 2], [0, 2], [1, 3]]]
    for ns, n in ((5, 10), (10, 420), (20, 9690)):
        q = observation.closure_quadrangles(ns)
        assert q.shape == (n, 4, 2) and (q[:, :, 0] < q[:, :, 1]).all()
        # every quadrangle closes: each of its four stations sits once in the numerator and once in the denominator
        for row in q[:: max(1, n // 50)]:
            assert sorted(row[:2].ravel()) == sorted(row[2:].ravel()) and len(set(row.ravel().tolist())) == 4
    c = K.case('12x20')
    pairs = {tuple(p): i for i, p in enumerate(c['pairs'].tolist())}
    want = np.array([[pairs[tuple(leg)] for leg in row] for row in c['quadrangles'].tolist()])
    assert c['quad'].dtype == np.int32 and c['quad'].shape == (10, 4) and np.array_equal(c['quad'], want)
    # either orientation of a stored baseline serves: amplitudes do not see it
    rev = c['pairs'].copy()
    rev[3] = rev[3][::-1]
    assert np.array_equal(observation.quadrangle_table(rev, c['quadrangles']), want)
    with pytest.raises(ValueError, match='baseline'):
        observation.quadrangle_table(np.delete(c['pairs'], 3, axis=0), c['quadrangles'])
    with pytest.raises(AttributeError):                                # an index outside the baselines
        observation.ClosureDFT(c['uv'], E.FOV, 8, quadrangles=np.array([[0, 1, 2, 10]]))
    with pytest.raises(AttributeError):                                # not (nca, 4)
        observation.ClosureDFT(c['uv'], E.FOV, 8, quadrangles=np.array([[0, 1, 2]]))
    with pytest.raises(AttributeError):
        observation.ClosureDFT(c['uv'], E.FOV, 8, weights={'logcamp': -1.0})
    with pytest.raises(AttributeError):
        observation.ClosureDFT(c['uv'], E.FOV, 8, weights={'vis': 1.0})


def test_closure_quantities_pack_and_split():
    c = K.case('12x20', 2)
    op = K.operator(c, 'amp+cphase+logcamp', weights={'logcamp': 0.5})
    assert isinstance(op, observation.DirectDFT) and (op.nvis, op.ncp, op.nca) == (10, 10, 10)
    assert op.weights == {'amp': 1.0, 'cphase': 1.0, 'logcamp': 0.5}
    vis = c['vis']
    cp, lca = op.closure_phases(vis), op.log_closure_amplitudes(vis)
    assert cp.dtype == np.float64 and lca.dtype == np.float64 and cp.shape == lca.shape == vis.shape[:-1] + (10,)
    assert np.array_equal(cp, E.closure_phases(vis, c['tri'], c['sign']))
    a = np.abs(vis)
    q = c['quad']
    assert np.allclose(lca, np.log(a[..., q[:, 0]] * a[..., q[:, 1]] / (a[..., q[:, 2]] * a[..., q[:, 3]])), rtol=0, atol=1e-12)
    # a station gain g_i on every visibility V_ij -> g_i conj(g_j) V_ij leaves both closure quantities unchanged
    rng = np.random.default_rng(0)
    g = rng.uniform(0.5, 2.0, c['ns']) * np.exp(1j * rng.uniform(-3, 3, c['ns']))
    corrupted = vis * g[c['pairs'][:, 0]] * np.conj(g[c['pairs'][:, 1]])
    assert np.abs(op.log_closure_amplitudes(corrupted) - lca).max() < 1e-12
    assert np.abs(np.angle(np.exp(1j * (op.closure_phases(corrupted) - cp)))).max() < 1e-12
    both = op.pack({'logcamp': lca, 'cphase': cp})                      # the canonical order, whatever the dict's
    assert both.shape == vis.shape[:-1] + (20,) and np.array_equal(both[..., :10], cp) and np.array_equal(both[..., 10:], lca)
    back = op.split(both, 'cphase+logcamp')
    assert list(back) == ['cphase', 'logcamp'] and np.array_equal(back['cphase'], cp) and np.array_equal(back['logcamp'], lca)
    with pytest.raises(AttributeError):                                # 20 entries: amp+cphase, amp+logcamp or cphase+logcamp
        op.split(both)
    three = op.pack({'amp': a, 'cphase': cp, 'logcamp': lca})
    assert list(op.split(three)) == ['amp', 'cphase', 'logcamp'] and np.array_equal(op.split(three)['amp'], a)
    nine = K.operator(K.case('9x11'), 'cphase+logcamp')
    assert (nine.nvis, nine.ncp, nine.nca) == (45, 120, 420)
    assert [(k, v.shape[-1]) for k, v in nine.split(np.zeros((1, 540))).items()] == [('cphase', 120), ('logcamp', 420)]
    with pytest.raises(AttributeError):
        op.pack({'cphase': cp[..., :9]})
    with pytest.raises(AttributeError):
        op.pack({'vis': vis})
    with pytest.raises(AttributeError):
        op.split(both[..., :19], 'cphase+logcamp')
    with pytest.raises(AttributeError):
        K.operator(c, 'cphase').pack({'logcamp': lca})                 # no quadrangle table


def test_take_and_to_keep_the_type_the_tables_and_the_weights():
    import torch
    from bhnerf_amd import optimization, units
    c = K.case('12x20')
    op = K.operator(c, 'cphase+logcamp', weights={'cphase': 2.0})
    sub = op.take([2, 0])
    assert type(sub) is observation.ClosureDFT and sub.shape == (2, 10, 2) and sub.uv.dtype == np.float64
    assert sub.uv.tobytes() == c['uv'][[2, 0]].tobytes() and sub.quad is op.quad and sub.tri is op.tri and sub.weights == op.weights
    moved = op.to('cpu')
    assert type(moved) is observation.ClosureDFT and isinstance(moved.quad, torch.Tensor) and moved.quad.dtype == torch.int32
    assert np.array_equal(moved.quad.numpy(), c['quad']) and np.array_equal(moved.tri.numpy(), c['tri']) and moved.weights == op.weights
    again = moved.take(torch.tensor([1]))
    assert type(again) is observation.ClosureDFT and again.quad is moved.quad and (again.nca, again.ncp) == (10, 10)
    assert type(observation.ClosureDFT(c['uv'], E.FOV, 8, quadrangles=moved.quad).quad) is torch.Tensor      # a device table is handed on
    # a plain DirectDFT stays what it is
    plain = E.operator(c, 'cphase')
    assert type(plain.take([0])) is observation.DirectDFT and not hasattr(plain, 'quad')
    # TemporalBatchedArgs batches the subclass through .take; TrainStep.eht_closure builds one loss
    t_frames = np.arange(c['B']) * 0.1 * units.hr
    data = {'logcamp': c['data']['logcamp'], 'cphase': (c['data']['cphase'][0], 0.1)}
    step = optimization.TrainStep.eht_closure(t_frames, c['uv'], E.FOV, (12, 20), c['pairs'], data, weights={'logcamp': 0.5}, scale=2.0)
    assert step.num_losses == 1 and str(step.dtype[0]) == 'cphase+logcamp' and float(step.scale[0]) == 2.0
    tgt, sig, held = step.args[0].host_args
    assert type(held) is observation.ClosureDFT and (held.ncp, held.nca) == (10, 10) and held.weights['logcamp'] == 0.5
    assert np.array_equal(tgt, K.packed(c, 'cphase+logcamp')[0]) and np.all(sig[:, :10] == np.float32(0.1))
    assert np.array_equal(sig[:, 10:], c['data']['logcamp'][1])
    got = step.args[0][[2, 0]][2]
    assert type(got) is observation.ClosureDFT and got.shape == (2, 10, 2)
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_closure(t_frames, c['uv'], E.FOV, (12, 20), c['pairs'], {'vis': (0, 1)})
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_closure(t_frames, c['uv'], E.FOV, (12, 20), c['pairs'], {})


def test_closure_terms_parses_the_canonical_order_only():
    from bhnerf_amd import engine
    for d in K.DTYPES:
        assert engine.closure_terms(d) == tuple(d.split('+'))
    for bad in ('vis', 'vis+amp', 'logcamp+cphase', 'cphase+amp', 'amp+amp', '', 'amp+', '+amp', 'camp', 'amp + cphase', None, 3):
        assert engine.closure_terms(bad) is None, bad
    assert engine.EHT_DTYPES == {'vis': 0, 'amp': 1, 'cphase': 2}


@pytest.mark.parametrize('name,Sx', K.PARAMS)
def test_reference_amp_and_cphase_parts_equal_the_table_form_of_the_uv_tests(name, Sx):
    c = K.case(name, Sx)
    assert c['min_amp'] >= E.MIN_AMP, c['min_amp']
    print('\n[closure] %s Sx %d: smallest |vis| / largest = %.3f' % (name, Sx, c['min_amp']))
    total, grad, parts, vis = K.reference(c, 'amp+cphase+logcamp', K.WEIGHTS, 2.0)
    assert np.array_equal(vis, c['vis']) or np.abs(vis - c['vis']).max() < 1e-12
    sums = 0.0
    for d in ('amp', 'cphase'):
        loss, g, _ = E.table_loss(c['images'], c['A128'], *c['data'][d], 1.0, d, c['tri'], c['sign'])
        one = K.reference(c, d)
        assert abs(one[0] - loss) <= 1e-12 * abs(loss) and E.rel_max(one[1], g) < 1e-12, d
        assert abs(parts[d] - 2.0 * K.WEIGHTS[d] * loss) <= 1e-12 * abs(parts[d])
        sums = sums + 2.0 * K.WEIGHTS[d] * g
    # the weighted sum is linear in its terms, the gradient with it
    lca = K.reference(c, 'logcamp')
    assert abs(total - sum(parts.values())) <= 1e-12 * abs(total)
    assert E.rel_max(grad, sums + 2.0 * K.WEIGHTS['logcamp'] * lca[1]) < 1e-10
    # the logcamp reference against plain NumPy on the float64 visibilities
    op = K.operator(c, 'logcamp')
    t, s = c['data']['logcamp']
    want = (((op.log_closure_amplitudes(c['vis']) - t.astype(np.float64)) / s.astype(np.float64)) ** 2).sum()
    assert abs(lca[0] - want) <= 1e-12 * want
    print('[closure] %s Sx %d: chi^2 amp %.4e cphase %.4e logcamp %.4e, rms logcamp residual / sigma %.1f'
          % (name, Sx, K.reference(c, 'amp')[0], K.reference(c, 'cphase')[0], want, np.sqrt(want / t.size)))


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/eht_closure_host.cpp built with the sanitizers -> run(case, dtype, ...) -> (vis, loss[4], dimages or None)."""
    exe, work = side.build_host_program(tmp_path_factory, 'eht_closure_host')

    def run(c, dtype, want_grad=True, scale=1.0, weights=None, tag='case'):
        terms = dtype.split('+')
        H, W, B, Sx = c['H'], c['W'], c['B'], max(c['Sx'], 1)
        N, nvis = B * Sx, len(c['pairs'])
        ncp = len(c['tri']) if 'cphase' in terms else 0
        nca = len(c['quad']) if 'logcamp' in terms else 0
        w = dict({t: 1.0 for t in K.TERMS}, **(weights or {}))
        present = sum(1 << K.TERMS.index(t) for t in terms)
        head = np.array([N, Sx, nvis, ncp, nca, H, W, present, int(want_grad), E.FOV / W, E.FOV / H, scale] + [w[t] for t in K.TERMS],
                        dtype=np.float64)
        arrays = [head, c['uv'], c['images']]
        for t in terms:
            arrays += [c['data'][t][0].astype(np.float32), c['data'][t][1].astype(np.float32)]
        arrays += ([c['tri'], c['sign']] if ncp else []) + ([c['quad']] if nca else [])
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        with open(fin, 'wb') as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        npix = N * H * W
        assert len(raw) == 8 * N * nvis + 16 + (4 * npix if want_grad else 0)         # the documented sizes, nothing else
        vis = np.frombuffer(raw, dtype=np.complex64, count=N * nvis).reshape(c['images'].shape[:-2] + (nvis,))
        loss = np.frombuffer(raw, dtype=np.float32, count=4, offset=8 * N * nvis)
        dimg = np.frombuffer(raw, dtype=np.float32, count=npix, offset=8 * N * nvis + 16).reshape(c['images'].shape) if want_grad else None
        return vis, loss, dimg
    return run


@pytest.mark.parametrize('name,Sx', K.PARAMS)
def test_host_build_meets_the_float64_reference_on_every_term_combination(host_program, name, Sx):
    c = K.case(name, Sx)
    assert c['min_amp'] >= E.MIN_AMP
    for dtype in K.DTYPES:
        terms = dtype.split('+')
        ref = K.reference(c, dtype, K.WEIGHTS, 2.0)
        vis, loss, dimg = host_program(c, dtype, scale=2.0, weights=K.WEIGHTS, tag='%s_%d_%s' % (name, Sx, dtype))
        assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss).all()     # every element written
        assert E.rel_max(vis, c['vis']) <= E.F32_TOL
        parts = {t: float(loss[1 + K.TERMS.index(t)]) for t in terms}
        assert all(loss[1 + K.TERMS.index(t)] == 0 for t in K.TERMS if t not in terms)                             # absent terms are 0
        assert loss[0] == np.float32(np.float32(loss[1] + loss[2]) + loss[3])                                      # added in that order
        err = K.errors(dtype, float(loss[0]), parts, dimg, ref)
        print('\n[closure, host build] %s Sx %d %-18s %s' % (name, Sx, dtype, '  '.join('%s %.1e' % kv for kv in err.items())), end='')
        for t in terms:
            assert err[t] <= bound([t]), (dtype, t, err)
        assert err['total'] <= bound(terms) and err['dimages'] <= bound(terms), (dtype, err)
        # forward only: the same loss, the same visibilities
        vis0, loss0, none = host_program(c, dtype, want_grad=False, scale=2.0, weights=K.WEIGHTS, tag='nograd')
        assert none is None and loss0.tobytes() == loss.tobytes() and vis0.tobytes() == vis.tobytes()
    print()


def test_host_build_scale_and_weight_enter_as_one_effective_scale(host_program):
    """scale 2, w 1 and scale 1, w 2 are the same effective scale: the same bits.  Weight 1 changes no bit of a single term."""
    c = K.case('12x20')
    for dtype in ('logcamp', 'cphase+logcamp', 'amp+cphase+logcamp'):
        terms = dtype.split('+')
        _, la, da = host_program(c, dtype, scale=2.0, tag='s2')
        _, lb, db = host_program(c, dtype, scale=1.0, weights={t: 2.0 for t in terms}, tag='w2')
        assert la.tobytes() == lb.tobytes() and da.tobytes() == db.tobytes(), dtype
        _, l1, d1 = host_program(c, dtype, tag='s1')
        assert np.abs(la - 2 * l1).max() <= 1e-6 * abs(la[0]) and np.abs(da - 2 * d1).max() <= 1e-6 * np.abs(da).max()
    # a term at weight 0 is present and contributes exactly nothing
    _, l0, d0 = host_program(c, 'cphase+logcamp', weights={'logcamp': 0.0}, tag='w0')
    _, lc, dc = host_program(c, 'cphase', tag='c')
    assert l0[3] == 0 and l0[0] == lc[0] == l0[2] and np.array_equal(d0, dc)


def test_host_build_zero_amplitude_rule(host_program):
    """An all-zero plane has |V| = 0 on every baseline: 'logcamp' contributes 0 to the loss and a zero gradient there, not NaN
    or infinity, and the other planes are what they are without it."""
    full = K.case('13x7')
    c = dict(full, images=full['images'].copy())
    c['images'][0] = 0.0
    vis, loss, dimg = host_program(c, 'logcamp', tag='zero')
    assert not vis[0].any() and np.isfinite(loss).all() and not dimg[0].any() and dimg[1].any()
    _, lfull, dfull = host_program(full, 'logcamp', tag='full')
    assert np.array_equal(dimg[1], dfull[1]) and 0 < loss[3] < lfull[3]
    c['images'][1] = 0.0
    for dtype in ('logcamp', 'cphase+logcamp', 'amp+cphase+logcamp'):
        vis, loss, dimg = host_program(c, dtype, tag='zero_' + dtype)
        assert not vis.any() and np.isfinite(loss).all() and loss[3] == 0 and not dimg.any(), dtype


def test_argument_validation_returns_before_any_device_call():
    import ctypes as C
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.cls_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    N, Sx, nvis, ncp, nca, H, W = 4, 2, 10, 10, 10, 12, 20
    need = lib.bhn_cls_ws_bytes(N, nvis, ncp, nca, H, W)
    assert need > 0 and need % 256 == 0 and lib.bhn_cls_ws_bytes(N, nvis, 0, 0, H, W) < need
    assert lib.bhn_cls_ws_bytes(N, nvis, ncp, 0, H, W) > _hip.eht_lib().bhn_eht_ws_bytes(N, nvis, ncp, H, W)
    for bad in ((0, nvis, ncp, nca, H, W), (N, 0, ncp, nca, H, W), (N, nvis, -1, nca, H, W), (N, nvis, ncp, -1, H, W), (N, nvis, ncp, nca, 0, W),
                (N, nvis, ncp, nca, H, 0)):
        assert lib.bhn_cls_ws_bytes(*bad) == 0
    term = lambda **kw: _hip.bhn_cls_term(**dict(dict(target=4096, sigma=4096, weight=1.0), **kw))
    good = dict(images=p, uv=p, N=N, Sx=Sx, nvis=nvis, H=H, W=W, psize_x=1e-11, psize_y=1e-11, amp=term(), cphase=term(), logcamp=term(),
                tri=p, tri_sign=p, ncp=ncp, quad=p, nca=nca, scale=1.0, loss=p, dimages=p, ws=p, ws_bytes=need)
    order = list(good)
    bad = [(dict(images=None), b'null', 1), (dict(uv=None), b'null', 1), (dict(loss=None), b'null', 1), (dict(ws=None), b'null', 1),
           (dict(amp=None, cphase=None, logcamp=None), b'no term present', 1),
           (dict(amp=term(target=None)), b"'amp' with a null", 1), (dict(cphase=term(sigma=None)), b"'cphase' with a null", 1),
           (dict(logcamp=term(target=None)), b"'logcamp' with a null", 1), (dict(logcamp=term(weight=-0.5)), b'weight', 1),
           (dict(amp=term(weight=float('inf'))), b'weight', 1), (dict(cphase=term(weight=float('nan'))), b'weight', 1),
           (dict(tri=None), b'triangle table', 1), (dict(tri_sign=None), b'triangle table', 1), (dict(ncp=0), b'triangle table', 1),
           (dict(ncp=-1), b'triangle table', 1), (dict(quad=None), b'quadrangle table', 1), (dict(nca=0), b'quadrangle table', 1),
           (dict(nca=-3), b'quadrangle table', 1), (dict(N=0), b'sizes below 1', 1), (dict(nvis=0), b'sizes below 1', 1),
           (dict(H=0), b'sizes below 1', 1), (dict(W=-2), b'sizes below 1', 1), (dict(Sx=0), b'sizes below 1', 1), (dict(Sx=3), b'multiple of Sx', 1),
           (dict(psize_x=0.0), b'pixel sizes', 1), (dict(psize_y=float('nan')), b'pixel sizes', 1),
           (dict(cphase=None, ncp=-1), b'ncp must be', 1), (dict(logcamp=None, nca=-1), b'nca must be', 1),
           (dict(ws=C.c_void_p(4100)), b'aligned', 1), (dict(uv=C.c_void_p(4100)), b'aligned', 1),
           (dict(ws_bytes=need - 1), b'workspace of', _hip.BHN_EWORKSPACE), (dict(ws_bytes=0), b'workspace of', _hip.BHN_EWORKSPACE)]
    for change, word, code in bad:
        a = dict(good, **change)
        args = [C.byref(a[k]) if isinstance(a[k], _hip.bhn_cls_term) else a[k] for k in order]
        rc = lib.bhn_cls_chi2(*args, None)
        assert rc == code, (change, rc, lib.bhn_cls_last_error())
        msg = lib.bhn_cls_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_cls'):
            _hip.cls_check(rc)
    _hip.cls_check(0)


CLS_NAMES = ['bhn_cls_chi2', 'bhn_cls_last_error', 'bhn_cls_ws_bytes']


def test_cls_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_cls.so: the dynamic symbol table is the declarations of include/bhnerf_cls.h and nothing else, the ctypes table
    binds exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or
    ctypes table knows a name that begins with bhn_cls.  The eighth library has a tuple of its own: _hip.LIBRARIES keeps its five
    keys, and libbhnerf_eht.so keeps its four symbols."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_cls.h'))))
    assert declared == sorted(_hip.CLS_SIGNATURES) == CLS_NAMES
    defined = side._symbols(_hip.CLS_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.CLS_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.CLS_LIBRARY == (_hip.CLS_LIB_PATH, _hip.CLS_SIGNATURES, 'bhn_cls_last_error', None)
    assert len(_hip.CLS_LIBRARY) == len(_hip.FLOW_LIBRARY) and [type(v) for v in _hip.CLS_LIBRARY] == [type(v) for v in _hip.FLOW_LIBRARY]
    assert _hip.cls_lib() is _hip.load(_hip.CLS_LIB_PATH, _hip.CLS_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    others += [('bhnerf_flow.h',) + _hip.FLOW_LIBRARY[:2], ('bhnerf_rec.h',) + _hip.REC_LIBRARY[:2]]
    assert len(others) == 7
    for other_header, path, table in others:
        assert 'bhn_cls' not in side._header(other_header), other_header
        assert 'bhn_cls' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_cls') for k in table), other_header
    eht = side._symbols(_hip.EHT_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in eht.splitlines() if line.strip()) == sorted(_hip.EHT_SIGNATURES)


def test_combined_dtypes_need_the_closure_operator():
    """Every AttributeError that needs no device: a combined dtype, or 'logcamp', on a plain DirectDFT or on dense matrices, and on a
    ClosureDFT a dtype it has no table for, 'vis', a wrong last axis."""
    import torch
    from bhnerf_amd import engine
    c = K.case('12x20')
    img = torch.as_tensor(c['images'])
    tgt, sig = K.packed(c, 'cphase+logcamp')
    for op in (E.operator(c, 'cphase'), E.operator(c, 'amp')):
        for dtype in ('cphase+logcamp', 'logcamp', 'amp+cphase'):
            with pytest.raises(AttributeError):
                engine.chi2_eht(img, op, tgt, sig, 1.0, dtype)
    with pytest.raises(AttributeError):                                # dense matrices know no 'logcamp'
        engine.chi2_eht(img.reshape(3, -1), E.operator(c, 'amp').dense(), c['data']['logcamp'][0], c['data']['logcamp'][1], 1.0, 'logcamp')
    # the training step's body and loss_fn_eht refuse them at their first line: a combined dtype needs the operator that carries its tables
    from bhnerf_amd import network, units
    for A in (E.operator(c, 'cphase'), E.operator(c, 'amp').dense()):
        for dtype in ('cphase+logcamp', 'logcamp'):
            with pytest.raises(AttributeError, match='not supported'):
                network.test_eht(None, units.hr, dtype, tgt, sig, A, *([None] * 10), 1.0)
            with pytest.raises(AttributeError, match='not supported'):
                network.gradient_step_eht(None, units.hr, dtype, tgt, sig, A, *([None] * 10), 1.0)
    closed = K.operator(c, 'cphase+logcamp')
    with pytest.raises(AttributeError, match='not supported'):
        network.test_eht(None, units.hr, 'logcamp+cphase', tgt, sig, closed, *([None] * 10), 1.0)
    with pytest.raises(AttributeError, match='quadrangles'):           # no quadrangle table
        engine.chi2_eht(img, K.operator(c, 'cphase'), tgt, sig, 1.0, 'cphase+logcamp')
    with pytest.raises(AttributeError, match='triangles'):             # no triangle table
        engine.chi2_eht(img, K.operator(c, 'logcamp'), tgt, sig, 1.0, 'cphase+logcamp')
    for dtype in ('vis', 'logcamp+cphase', 'nope'):
        with pytest.raises(AttributeError, match='not supported'):
            engine.chi2_eht(img, closed, tgt, sig, 1.0, dtype)
    with pytest.raises(AttributeError, match='should end in 20'):      # the last axis
        engine.chi2_eht(img, closed, tgt[:, :19], sig[:, :19], 1.0, 'cphase+logcamp')
    with pytest.raises(AttributeError, match='should end in 10'):
        engine.chi2_eht(img, closed, tgt, sig, 1.0, 'logcamp')
