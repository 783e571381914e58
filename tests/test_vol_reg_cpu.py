"""CPU tests of the volume priors (libbhnerf_reg.so, csrc/vol_reg.hip, regularization.VolumePrior): everything about them that
needs no device.

The plan and the per-voxel arithmetic live in csrc/vol_reg.h and compile with a plain C++ compiler.  tools/vol_reg_host.cpp walks
the launches of bhn_reg_loss one workgroup after the other; here it is built with g++ -O2 and the sanitizers
(tests/side_lib_support.py), run as a child process with its inputs, outputs and workspace in heap blocks of exactly the
documented sizes, and compared with the float64 reference of tests/vol_reg_cases.py.  Nothing built with a sanitizer is loaded
into this Python process.

Bound: the project's f32 bound, eht_uv_cases.F32_TOL = 2e-5: the loss slots relative, the gradient relative to its largest
element.  The figures are printed.  The five wrong variants of the reference must stand out by five times that bound."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
import side_lib_support as side                                        # noqa: E402
import vol_reg_cases as R                                              # noqa: E402

TOL = E.F32_TOL


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/vol_reg_host.cpp built with the sanitizers -> run(case, ...) -> (loss[4], per_volume (3, N) or None, grad or None)."""
    exe, work = side.build_host_program(tmp_path_factory, 'vol_reg_host')

    def run(c, want_grad=True, want_pv=True, tag='case', status=0):
        e, mask = c['e'], c['mask']
        N, dims = e.shape[0], e.shape[1:]
        head = np.array([N, *dims, int(mask is not None), int(want_grad), int(want_pv), *c['spacing'], *c['weights'], c['eps'], c['scale']],
                        dtype=np.float64)
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        with open(fin, 'wb') as f:
            for a in [head, e.astype(np.float32)] + ([mask.astype(np.uint8)] if mask is not None else []):
                f.write(np.ascontiguousarray(a).tobytes())
        if status:
            import subprocess
            res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
            assert res.returncode == status, (res.returncode, res.stderr[-2000:])
            return res.stderr
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        assert len(raw) == 16 + (12 * N if want_pv else 0) + (4 * e.size if want_grad else 0)     # the documented sizes, nothing else
        loss = np.frombuffer(raw, dtype=np.float32, count=4)
        pv = np.frombuffer(raw, dtype=np.float32, count=3 * N, offset=16).reshape(3, N) if want_pv else None
        grad = np.frombuffer(raw, dtype=np.float32, count=e.size, offset=16 + (12 * N if want_pv else 0)).reshape(e.shape) if want_grad else None
        return loss, pv, grad
    return run


_REFS = {}


def ref_of(name, weights=None):
    """The float64 reference of a case, computed once."""
    key = (name, weights)
    if key not in _REFS:
        c = R.make_case(name)
        if weights is not None:
            c = dict(c, weights=weights)
        _REFS[key] = (c, R.reference(c['e'], c['mask'], c['spacing'], c['weights'], c['eps'], c['scale']))
    return _REFS[key]


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_host_build_meets_the_float64_reference(host_program, name):
    c, (loss_ref, pv_ref, grad_ref) = ref_of(name)
    loss, pv, grad = host_program(c, tag=name)
    assert np.isfinite(loss).all() and np.isfinite(pv).all() and np.isfinite(grad).all()        # every element written
    le, pe, ge = R.loss_error(loss, loss_ref), R.loss_error(pv, pv_ref), R.grad_error(grad, grad_ref)
    print('%s: loss %.2e per_volume %.2e gradient %.2e' % (name, le, pe, ge))
    assert le < TOL and pe < TOL and ge < TOL
    if c['mask'] is not None:
        assert not grad[:, c['mask'] == 0].any()                     # exactly 0 outside the mask
    # without the optional outputs: the same loss, bit for bit
    loss2, pv2, grad2 = host_program(c, want_grad=False, want_pv=False, tag=name + '_bare')
    assert pv2 is None and grad2 is None and loss2.tobytes() == loss.tobytes()


@pytest.mark.parametrize('weights', R.SINGLE_WEIGHTS)
@pytest.mark.parametrize('name', ('5x7x3', '33x17x9'))
def test_single_terms_and_absent_slots(host_program, name, weights):
    c, (loss_ref, pv_ref, grad_ref) = ref_of(name, weights)
    full = host_program(R.make_case(name), tag=name + '_full')
    loss, pv, grad = host_program(dict(c, eps=c['eps'] if weights[0] else 0.0), tag=name + '_single')     # no tv: no requirement on eps
    d = weights.index(1.0)
    for other in set(range(3)) - {d}:
        assert loss[1 + other] == 0.0 and not pv[other].any()        # an absent term: exactly 0
    assert pv[d].tobytes() == full[1][d].tobytes()                   # the present one: the bits it has among all three
    assert loss[0] == loss[1 + d]
    assert R.loss_error(loss, loss_ref) < TOL and R.grad_error(grad, grad_ref) < TOL


@pytest.mark.parametrize('name', ('5x7x3', 'no_mask'))
def test_all_weights_zero_is_all_zero(host_program, name):
    c = dict(R.make_case(name), weights=(0.0, 0.0, 0.0), eps=float('nan'))
    loss, pv, grad = host_program(c, tag=name + '_zero')
    assert not loss.any() and not pv.any() and not grad.any()


def test_masked_out_contents_change_no_bit(host_program):
    c = R.make_case('13x7x11')
    out = host_program(c, tag='clean')
    junk = c['e'].copy()
    junk[:, c['mask'] == 0] = np.array([np.nan, np.inf, -3e38, 7.0], dtype=np.float32)[np.arange(int((c['mask'] == 0).sum())) % 4]
    out2 = host_program(dict(c, e=junk), tag='junk')
    for a, b in zip(out, out2):
        assert a.tobytes() == b.tobytes()


def test_closed_forms_of_the_tiny_cases(host_program):
    s, (wtv, wtsv, wl1), eps, (hx, hy, hz) = R.SCALE, R.WEIGHTS, R.EPS, R.SPACING
    # 1x1x1: no difference exists: tv = eps, tsv = 0, l1 = e, the gradient is that of l1
    c = R.make_case('1x1x1')
    e0 = float(c['e'].ravel()[0])
    loss, pv, grad = host_program(c, tag='tiny1')
    assert e0 > 0
    np.testing.assert_allclose(pv[:, 0], [eps, 0.0, e0], rtol=TOL, atol=0)
    np.testing.assert_allclose(grad.ravel(), [s * wl1], rtol=TOL)
    np.testing.assert_allclose(loss, [s * (wtv * eps + wl1 * e0), s * wtv * eps, 0.0, s * wl1 * e0], rtol=TOL)
    # 2x1x1: one difference, stored at voxel 0
    c = R.make_case('2x1x1')
    a, b = (float(v) for v in c['e'].ravel())
    dx = (b - a) / hx
    root = np.sqrt(dx * dx + eps * eps)
    loss, pv, grad = host_program(c, tag='tiny2')
    np.testing.assert_allclose(pv[:, 0], [root + eps, dx * dx, a + b], rtol=TOL)
    t = dx * (wtv / root + 2 * wtsv) / hx
    np.testing.assert_allclose(grad.ravel(), [s * (-t + wl1), s * (t + wl1)], rtol=TOL)
    # 1x1x5, two volumes: a chain along z, each volume on its own
    c = R.make_case('1x1x5')
    loss, pv, grad = host_program(c, tag='tiny5')
    for n in range(2):
        v = c['e'][n].ravel().astype(np.float64)
        dz = np.diff(v) / hz
        np.testing.assert_allclose(pv[:, n], [np.sqrt(dz ** 2 + eps ** 2).sum() + eps, (dz ** 2).sum(), v.sum()], rtol=TOL)
        t = np.concatenate([dz * (wtv / np.sqrt(dz ** 2 + eps ** 2) + 2 * wtsv) / hz, [0.0]])
        want = s * (-t + np.concatenate([[0.0], t[:-1]]) + wl1)
        assert np.abs(grad[n].ravel() - want).max() < TOL * np.abs(want).max()
    # sign(0) = 0: a zero voxel with zero differences has zero gradient
    z = dict(R.make_case('1x1x1'), e=np.zeros((1, 1, 1, 1), dtype=np.float32))
    assert host_program(z, tag='zero')[2].ravel()[0] == 0.0


@pytest.mark.parametrize('name', R.MUTANT_CASES)
def test_mutants_of_the_reference_stand_out(name):
    c, (_, _, grad_ref) = ref_of(name)
    moves = {}
    for mutant in R.MUTANTS:
        grad = R.reference(c['e'], c['mask'], c['spacing'], c['weights'], c['eps'], c['scale'], mutant=mutant)[2]
        moves[mutant] = R.grad_error(grad, grad_ref)
    print(name, ' '.join('%s %.2e' % kv for kv in moves.items()))
    assert len(moves) == 5 and min(moves.values()) >= 5 * TOL, moves


def test_host_program_refuses_what_the_library_refuses(host_program):
    c = R.make_case('5x7x3')
    assert 'eps' in host_program(dict(c, eps=0.0), tag='bad_eps', status=1)
    assert 'spacing' in host_program(dict(c, spacing=(0.5, 0.0, 1.0)), tag='bad_h', status=1)
    assert 'weights' in host_program(dict(c, weights=(1.0, -1.0, 0.0)), tag='bad_w', status=1)
    assert 'scale' in host_program(dict(c, scale=float('inf')), tag='bad_s', status=1)


def test_argument_validation_returns_before_any_device_call():
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.reg_lib()
    p = C.c_void_p(4096)                    # never dereferenced: every call below is refused before a launch
    N, nx, ny, nz = 2, 33, 17, 9
    need = lib.bhn_reg_ws_bytes(N, nx, ny, nz)
    assert need == 256 * 2 and need % 256 == 0          # 5 workgroups x 3 terms x 2 volumes of partial sums, and the (3, 2) sums
    assert lib.bhn_reg_ws_bytes(1, 64, 64, 64) == 3 * 256 * 4 + 256
    for bad in ((0, nx, ny, nz), (N, 0, ny, nz), (N, nx, -1, nz), (N, nx, ny, 0), (1, 2048, 2048, 512), (1, 65536, 65536, 1)):
        assert lib.bhn_reg_ws_bytes(*bad) == 0
    f3 = lambda *v: (C.c_float * 3)(*v)
    good = dict(volumes=p, N=N, nx=nx, ny=ny, nz=nz, mask=p, spacing=f3(1, 1, 1), weights=f3(1, 1, 1), eps=1e-3, scale=1.0, loss=p,
                per_volume=p, dvolumes=p, ws=p, ws_bytes=need)
    nan, inf = float('nan'), float('inf')
    bad = [(dict(volumes=None), b'null', 1), (dict(spacing=None), b'null', 1), (dict(weights=None), b'null', 1), (dict(loss=None), b'null', 1),
           (dict(ws=None), b'null', 1), (dict(N=0), b'at least 1', 1), (dict(nx=0), b'at least 1', 1), (dict(ny=-3), b'at least 1', 1),
           (dict(nz=0), b'at least 1', 1), (dict(nx=65536, ny=65536), b'too large', 1), (dict(spacing=f3(1, 0, 1)), b'spacing', 1),
           (dict(spacing=f3(-1, 1, 1)), b'spacing', 1), (dict(spacing=f3(1, 1, inf)), b'spacing', 1), (dict(spacing=f3(nan, 1, 1)), b'spacing', 1),
           (dict(weights=f3(1, -0.5, 1)), b'weights', 1), (dict(weights=f3(1, 1, inf)), b'weights', 1), (dict(weights=f3(nan, 1, 1)), b'weights', 1),
           (dict(scale=inf), b'scale', 1), (dict(scale=nan), b'scale', 1), (dict(eps=0.0), b'eps', 1), (dict(eps=-1.0), b'eps', 1),
           (dict(eps=nan), b'eps', 1), (dict(eps=inf), b'eps', 1), (dict(ws=C.c_void_p(4098)), b'aligned', 1),
           (dict(ws_bytes=need - 1), b'workspace of', _hip.BHN_EWORKSPACE), (dict(ws_bytes=0), b'workspace of', _hip.BHN_EWORKSPACE)]
    for change, word, code in bad:
        a = dict(good, **change)
        rc = lib.bhn_reg_loss(*[a[k] for k in good], None)
        assert rc == code, (change, rc, lib.bhn_reg_last_error())
        msg = lib.bhn_reg_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_reg'):
            _hip.reg_check(rc)
    _hip.reg_check(0)


REG_NAMES = ['bhn_reg_last_error', 'bhn_reg_loss', 'bhn_reg_ws_bytes']


def test_reg_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_reg.so: the dynamic symbol table is the declarations of include/bhnerf_reg.h and nothing else, the ctypes table
    binds exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or
    ctypes table knows a name that begins with bhn_reg.  The tenth library has a tuple of its own: _hip.LIBRARIES keeps its five
    keys."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', side._header('bhnerf_reg.h'))))
    assert declared == sorted(_hip.REG_SIGNATURES) == REG_NAMES
    defined = side._symbols(_hip.REG_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.REG_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.REG_LIBRARY == (_hip.REG_LIB_PATH, _hip.REG_SIGNATURES, 'bhn_reg_last_error', None)
    assert len(_hip.REG_LIBRARY) == len(_hip.POL_LIBRARY) and [type(v) for v in _hip.REG_LIBRARY] == [type(v) for v in _hip.POL_LIBRARY]
    assert _hip.reg_lib() is _hip.load(_hip.REG_LIB_PATH, _hip.REG_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    others += [('bhnerf_%s.h' % n,) + getattr(_hip, n.upper() + '_LIBRARY')[:2] for n in ('flow', 'rec', 'cls', 'pol')]
    assert len(others) == 9
    for other_header, path, table in others:
        assert 'bhn_reg' not in side._header(other_header), other_header
        assert 'bhn_reg' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_reg') for k in table), other_header
    # the kernels' code stands on the shared skeleton and on nothing of another library
    src = open(os.path.join(side.ROOT, 'bhnerf_amd', 'csrc', 'vol_reg.hip')).read()
    assert '#include "side_lib.h"' in src and not re.search(r'atomic\w*\s*\(', src)
    assert sorted(re.findall(r'#include "([^"]+)"', src)) == ['../../include/bhnerf_reg.h', 'side_lib.h', 'vol_reg.h']


def test_volume_prior_checks_its_arguments_before_any_launch():
    from bhnerf_amd import engine, network, optimization, regularization
    VP = regularization.VolumePrior
    assert regularization.REG_TERMS == ('tv', 'tsv', 'l1')
    op = VP(fov=20.0, resolution=(6, 5, 4), weights={'tv': 1.0, 'l1': 0.5})
    assert op.dims == (6, 5, 4) and op.weights == (1.0, 0.0, 0.5) and op.coords.shape == (3, 6, 5, 4, 1)
    np.testing.assert_allclose(op.spacing, (20.0 / 5, 20.0 / 4, 20.0 / 3))
    grid = np.linspace(-10.0, 10.0, 6)
    same = VP(coords=np.array(np.meshgrid(grid, grid, grid, indexing='ij')).astype(np.float32))
    assert same.dims == (6, 6, 6) and abs(same.spacing[0] - 4.0) < 1e-6
    np.testing.assert_array_equal(same.coords[..., 0], VP(fov=20.0, resolution=6).coords[..., 0])       # sample_3d_grid's lattice
    assert VP(fov=20.0).weights == (1.0, 0.0, 0.0) and VP(fov=20.0).dims == (64, 64, 64)
    assert VP(fov=20.0, weights={'tsv': 2.0}, eps=0.0).weights == (0.0, 2.0, 0.0)          # no tv: no requirement on eps
    warped = np.array(np.meshgrid(grid, grid ** 3, grid, indexing='ij'))
    for kw in (dict(), dict(fov=20.0, weights={'tvx': 1.0}), dict(fov=20.0, weights={'tv': -1.0}), dict(fov=20.0, weights={'l1': np.inf}),
               dict(fov=20.0, eps=0.0), dict(fov=20.0, eps=np.nan), dict(fov=20.0, resolution=0), dict(fov=20.0, resolution=(4, 4)),
               dict(fov=-1.0), dict(coords=warped), dict(coords=np.swapaxes(np.array(np.meshgrid(grid, grid, grid, indexing='ij')), 1, 2)),
               dict(coords=np.zeros((3, 4, 4))), dict(coords=np.array(np.meshgrid(grid[::-1], grid, grid, indexing='ij')))):
        with pytest.raises(AttributeError):
            VP(**kw)
    # engine.chi2_volume: shapes and the empty mask, on host tensors -- refused before the device is needed
    with pytest.raises(AttributeError, match='not volumes'):
        engine.chi2_volume(torch.zeros(6, 5, 3), op, 1.0)
    with pytest.raises(AttributeError, match='not volumes'):
        engine.chi2_volume(np.zeros((6, 5, 4), dtype=np.float32), op, 1.0)
    with pytest.raises(AttributeError, match='mask'):
        engine.chi2_volume(torch.zeros(2, 6, 5, 4), op, 1.0, mask=np.ones((6, 5, 5)))
    with pytest.raises(AttributeError, match='has none'):
        engine.chi2_volume(torch.zeros(6, 5, 4), op, 1.0, mask=np.zeros((6, 5, 4), dtype=np.uint8))
    half = np.zeros((6, 5, 4), dtype=np.uint8)
    half[:3] = 1
    assert op.call_weights(half) == (1.0 / 60, 0.0, 0.5 / 60) and op.call_weights(None) == (1.0 / 120, 0.0, 0.5 / 120)
    assert VP(fov=20.0, resolution=4, normalize=False).call_weights(np.zeros((4, 4, 4))) == (1.0, 0.0, 0.0)
    # the step: a static args object in the place of per-frame data
    step = optimization.TrainStep.volume_prior(20.0, resolution=4, weights={'tsv': 1.0}, scale=3.0)
    assert list(step.dtype) == ['volume'] and step.grad_pmap[0] is network.gradient_step_volume and step.test_pmap[0] is network.test_volume
    args = step.args[0]
    assert args.num_frames == 1 and not args.sample(5).any() and args.sample(5).shape == (5,)
    got = args[np.array([3, 1])]
    assert len(got) == 4 and got[0] is None and got[1] is None and got[2] is args[7][2] and isinstance(got[2], VP)
    both = optimization.TrainStep.image(np.arange(3.0), np.zeros((3, 4, 4)), dtype='full') + step
    assert both.num_losses == 2 and list(both.scale) == [1.0, 3.0] and both.args[0].num_frames == 3
    with pytest.raises(AttributeError):
        network.gradient_step_volume(None, None, 'full', None, None, got[2], *([None] * 10), 1.0)
    with pytest.raises(AttributeError):
        network.test_volume(None, None, 'volume', None, None, object(), *([None] * 10), 1.0)
    assert 'once per call' in optimization.TrainStep.volume_prior.__doc__.lower() and 'total_movie_loss' in optimization.TrainStep.volume_prior.__doc__
