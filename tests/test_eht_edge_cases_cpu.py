"""CPU proof that the edge-shape table of the (u, v) EHT kernels (tests/eht_edge_cases.py) can see what it is for; no device.

For every case: the float64 reference meets the admission conditions and the plan values its `why` claims (the Python restatement
of eht_make_plan is held to a C++ build of csrc/eht_uv.h, tools/eht_plan_host.cpp, and to the byte counts of the three libraries);
the reference with each listed mutant built in differs from the clean one by at least ten times the case's bound in every output
the mutant touches; and the stand-alone host programs (tools/eht_uv_host.cpp, eht_closure_host.cpp, eht_pol_host.cpp, built with
the sanitizers by the fixtures of the sibling CPU tests) meet the case's bound -- they hold the shared arithmetic of csrc/eht_uv.h
and none of the device-only code (waves, red[][], strides, column blocks), which separates the two when a device case fails."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closure_cases as K                                              # noqa: E402
import eht_edge_cases as T                                             # noqa: E402
import eht_uv_cases as E                                               # noqa: E402
import pol_cases as P                                                  # noqa: E402
import side_lib_support as side                                        # noqa: E402
from test_closure_cpu import host_program as cls_host                  # noqa: E402,F401
from test_eht_uv_cpu import host_program as uv_host                    # noqa: E402,F401
from test_pol_cpu import host_program as pol_host                      # noqa: E402,F401

NAMES = [c.name for c in T.CASES]
MARGIN = 10.0


def _forms(c):
    """(N, nvis, ncp, nca, H, W) of every form the case is run in."""
    out = [(c.B * max(Sx, 1), c.nvis, c.ncp, c.nca, c.H, c.W) for Sx in set(c.uv_Sx + c.cls_Sx)]
    if c.pol:
        H, W, B, _, ns = c.pol[0]
        out += [(B * Sx, ns * (ns - 1) // 2, 0, 0, H, W) for Sx in c.pol[1:]]
    return out


def test_plan_restatement_equals_the_cpp_plan_and_the_libraries(tmp_path_factory):
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    exe, _ = side.build_host_program(tmp_path_factory, 'eht_plan_host')
    sizes = [f for c in T.CASES for f in _forms(c)]
    # and a sweep across the thresholds of the row split and the block size
    sizes += [(1, nvis, 0, 0, H, W) for nvis in (1, 9, 190, 2100) for H in (1, 8, 9, 97, 512, 513, 520, 4097)
              for W in (1, 64, 65, 192, 193, 256, 257, 513)]
    for N, nvis, ncp, nca, H, W in sizes:
        res = subprocess.run([exe] + [str(v) for v in (N, nvis, ncp, nca, H, W)], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and not res.stderr.strip(), res.stderr
        kblocks, RS, rows_per, block, eht_bytes, cls_bytes, pol_bytes = (int(v) for v in res.stdout.split())
        p = T.plan(N, nvis, H, W)
        assert (p['kblocks'], p['RS'], p['rows_per'], p['block']) == (kblocks, RS, rows_per, block), (N, nvis, H, W, p, res.stdout)
        assert 1 <= RS <= T.EHT_MAX_SPLITS and (RS - 1) * rows_per < H <= RS * rows_per and 1 <= p['last_rows'] <= rows_per
        assert (p['trips'] - 1) * block < W <= p['trips'] * block and 1 <= p['tail_lanes'] <= T.WAVE
        assert eht_bytes == _hip.eht_lib().bhn_eht_ws_bytes(N, nvis, ncp, H, W) > 0
        assert cls_bytes == _hip.cls_lib().bhn_cls_ws_bytes(N, nvis, ncp, nca, H, W) > eht_bytes
        assert pol_bytes == _hip.pol_lib().bhn_pol_ws_bytes(N, nvis, H, W) > 0


def test_the_table_holds_the_siblings_bounds():
    import test_gpu_closure as TC
    assert T.CLS_LOGCAMP_BOUND == TC.LOGCAMP_BOUND
    for terms in (['amp'], ['cphase'], ['logcamp'], T.CLS_DTYPE.split('+')):
        for what in ('loss', 'dimages'):
            assert T.cls_bound(terms, what) == TC._bound(terms, what)
    assert T.pol_bound is P.bound and T.uv_bound('vis', 'loss') == E.F32_TOL == 2e-5
    assert sorted(T.BY_NAME) == sorted(['w65', 'w130', 'w256', 'w300', 'w513', 'h97_s20', 'h520', 's24', 'n260', 'turns', 'one'])
    assert all(set(T.CONTRACT) <= {n for n, _ in params} for params in (T.UV_PARAMS, T.CLS_PARAMS, T.POL_PARAMS))
    for name in ('w130', 'w300', 's24', 'n260'):           # the closure and pol builds run the cases that reach their own kernels
        assert T.BY_NAME[name].cls_Sx and T.BY_NAME[name].pol
    assert set(T.BY_NAME['w300'].pol[1:]) == set(T.BY_NAME['s24'].pol[1:]) == {3, 4}
    assert [sorted(T.MEASURED[k]) for k in ('uv', 'cls', 'pol')] == [sorted(T.UV_PARAMS), sorted(T.CLS_PARAMS), sorted(T.POL_PARAMS)]


@pytest.mark.parametrize('name', NAMES)
def test_admission_and_the_claimed_plan(name):
    c = T.BY_NAME[name]
    got = dict(T.plan(c.B, c.nvis, c.H, c.W), ncp=c.ncp, nca=c.nca)
    assert c.claims and all(got[k] == v for k, v in c.claims.items()), (c.claims, got)
    ratios = T.admitted(name)
    print('\n[eht edges] %-8s %s' % (name, '  '.join('%s %.3g' % (k, v) for k, v in ratios.items())))
    d = T.uv(name)
    assert d['images'].shape == (c.B, c.H, c.W) and len(d['pairs']) == c.nvis and len(d['tri']) == c.ncp and d['fov'] == c.fov


def _runs(c, mutant=None):
    """(label, bound of (terms, what), clean reference, mutated reference) of every form and dtype of the case."""
    for Sx in c.uv_Sx:
        for dtype in c.uv:
            yield ('uv Sx %d %s' % (Sx, dtype), lambda what: T.uv_bound(dtype, what), T.uv_reference(c.name, Sx, dtype),
                   T.uv_reference(c.name, Sx, dtype, mutant) if mutant else None)
    for Sx in c.cls_Sx:
        yield ('cls Sx %d' % Sx, lambda what: T.cls_bound(T.CLS_DTYPE.split('+'), what), T.cls_reference(c.name, Sx),
               T.cls_reference(c.name, Sx, mutant) if mutant else None)
    for Sx in (c.pol[1:] if c.pol else ()):
        yield ('pol Sx %d' % Sx, lambda what: T.pol_bound(T.POL_DTYPE.split('+'), what), T.pol_reference(c.name, Sx),
               T.pol_reference(c.name, Sx, mutant) if mutant else None)


@pytest.mark.parametrize('name', [c.name for c in T.CASES if c.mutants])
def test_every_listed_mutant_exceeds_the_bound_tenfold(name):
    c = T.BY_NAME[name]
    for mutant in c.mutants:
        for label, bound, clean, bad in _runs(c, mutant):
            diff = T.differences(clean, bad)
            touched = [k for k in T.MUTANTS[mutant] if k in diff]
            assert touched, (mutant, label)
            print('\n[eht edges] %-8s %-24s %-14s %s' % (name, mutant, label, '  '.join('%s %.1e' % (k, diff[k]) for k in touched)), end='')
            for what in touched:
                assert diff[what] > MARGIN * bound('loss' if what == 'loss' else 'dimages'), (mutant, label, what, diff)
    print()


def test_mutants_leave_alone_what_they_do_not_touch():
    """A slip of the adjoint or of a loss sum changes nothing else: the mutants are as narrow as the lines they stand for."""
    clean, bad = T.uv_reference('w300', 0, 'vis'), T.uv_reference('w300', 0, 'vis', 'adjoint_first_block_only')
    assert bad[0] == clean[0] and np.array_equal(bad[2], clean[2]) and np.array_equal(bad[1][..., :256], clean[1][..., :256])
    assert not bad[1][..., 256:].any() and clean[1][..., 256:].any()
    clean, bad = T.cls_reference('n260', 0), T.cls_reference('n260', 0, 'first_256_planes')
    assert np.array_equal(bad[1], clean[1]) and np.array_equal(bad[3], clean[3]) and 0 < bad[0] < clean[0]
    clean, bad = T.pol_reference('n260', 3), T.pol_reference('n260', 3, 'first_256_planes')
    assert np.array_equal(bad[1], clean[1]) and 0 < bad[0] < clean[0]


@pytest.mark.parametrize('name,Sx', T.UV_PARAMS)
def test_uv_host_program_meets_the_bound(uv_host, monkeypatch, name, Sx):
    c = T.BY_NAME[name]
    monkeypatch.setattr(E, 'FOV', c.fov)                                # the fixture takes the pixel size from eht_uv_cases.FOV ('turns')
    d = T.uv(name, Sx)
    for dtype in c.uv:
        ref_loss, ref_grad, ref_vis = T.uv_reference(name, Sx, dtype)
        vis, loss, dimg = uv_host(d, dtype, tag='%s_%d_%s' % (name, Sx, dtype))
        assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss)       # every element written
        e_vis, e_loss, e_grad = E.rel_max(vis, ref_vis), T.rel_loss(loss, ref_loss), T.rel_max(dimg, ref_grad)
        print('\n[eht edges, host build] uv  %-8s Sx %d %-6s vis %.1e loss %.1e dimages %.1e' % (name, Sx, dtype, e_vis, e_loss, e_grad), end='')
        assert e_vis <= E.F32_TOL and e_loss <= T.uv_bound(dtype, 'loss') and e_grad <= T.uv_bound(dtype, 'dimages'), (dtype, e_vis, e_loss, e_grad)
    if name == 'one':                                                   # the twiddles at the centre pixel are (1, 0)
        assert np.array_equal(vis.real, np.full(vis.shape, d['images'][0, 0, 0])) and not vis.imag.any()
    print()


@pytest.mark.parametrize('name,Sx', T.CLS_PARAMS)
def test_closure_host_program_meets_the_bound(cls_host, name, Sx):
    d, terms = T.cls(name, Sx), T.CLS_DTYPE.split('+')
    ref = T.cls_reference(name, Sx)
    vis, loss, dimg = cls_host(d, T.CLS_DTYPE, scale=T.CLS_SCALE, weights=K.WEIGHTS, tag='%s_%d' % (name, Sx))
    assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss).all()
    err = K.errors(T.CLS_DTYPE, float(loss[0]), {t: float(loss[1 + K.TERMS.index(t)]) for t in terms}, dimg, ref)
    print('\n[eht edges, host build] cls %-8s Sx %d %s' % (name, Sx, '  '.join('%s %.1e' % kv for kv in err.items())))
    assert E.rel_max(vis, d['vis']) <= E.F32_TOL
    for t in terms:
        assert err[t] <= T.cls_bound([t], 'loss'), (t, err)
    assert err['total'] <= T.cls_bound(terms, 'loss') and err['dimages'] <= T.cls_bound(terms, 'dimages'), err


@pytest.mark.parametrize('name,Sx', T.POL_PARAMS)
def test_pol_host_program_meets_the_bound(pol_host, name, Sx):
    d, terms = T.pol(name, Sx), T.POL_DTYPE.split('+')
    ref = T.pol_reference(name, Sx)
    vis, loss, dimg = pol_host(d, T.POL_DTYPE, scale=P.SCALE, weights=P.WEIGHTS, tag='%s_%d' % (name, Sx))
    assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(dimg).all() and np.isfinite(loss).all()
    err = P.errors(T.POL_DTYPE, float(loss[0]), {t: float(loss[1 + P.TERMS.index(t)]) for t in terms}, dimg, ref)
    print('\n[eht edges, host build] pol %-8s Sx %d %s' % (name, Sx, '  '.join('%s %.1e' % kv for kv in err.items())))
    assert E.rel_max(vis, d['vis']) <= E.F32_TOL
    for t in terms:
        assert err[t] <= T.pol_bound([t], 'loss'), (t, err)
    assert err['total'] <= T.pol_bound(terms, 'loss') and err['dimages'] <= T.pol_bound(terms, 'dimages'), err
