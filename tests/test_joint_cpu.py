"""CPU tests of the joint training step (optimization.TrainStep.joint, libbhnerf_jnt.so, csrc/joint_sum.hip): everything about it
that needs no device.

The argument checks, the plan of the launch and the per-element arithmetic live in csrc/joint_sum.h and compile with a plain C++
compiler.  tools/joint_sum_host.cpp walks the launch of bhn_jnt_sum one lane after the other; here it is built with g++ -O2 and the
sanitizers (tests/side_lib_support.py), run as a child process with every vector in a heap block of exactly its size, and compared
with NumPy's float32 left-to-right sum (tests/joint_cases.py).  Nothing built with a sanitizer is loaded into this Python process.

Every comparison is bitwise: a float32 left-to-right sum has one correct answer."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_cases as J                                                # noqa: E402
import side_lib_support as side                                        # noqa: E402


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/joint_sum_host.cpp built with the sanitizers -> run(srcs, losses, ...) -> (dst, loss_out or None, (vec, blocks)), or
    with `status` the program's stderr."""
    exe, work = side.build_host_program(tmp_path_factory, 'joint_sum_host')

    def run(srcs, losses, offset=0, alias=-1, want_losses=True, bad=0, K=None, n=None, status=0, tag='case'):
        K_file = len(srcs)
        K = K_file if K is None else K
        n_file = srcs.shape[1] if K_file else 0
        head = np.array([K, n_file if n is None else n, offset, alias, int(want_losses), bad], dtype=np.int64)
        fin, fout = str(work / (tag + '.in')), str(work / (tag + '.out'))
        with open(fin, 'wb') as f:
            for a in (head, np.ascontiguousarray(srcs, dtype=np.float32), np.ascontiguousarray(losses, dtype=np.float32)):
                f.write(a.tobytes())
        if status:
            res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
            assert res.returncode == status, (res.returncode, res.stderr[-2000:])
            return res.stderr
        side.run_host(exe, fin, fout)
        raw = open(fout, 'rb').read()
        assert len(raw) == 4 * n_file + (4 * (K + 1) if want_losses else 0) + 8          # the documented sizes, nothing else
        dst = np.frombuffer(raw, dtype=np.float32, count=n_file)
        loss_out = np.frombuffer(raw, dtype=np.float32, count=K + 1, offset=4 * n_file) if want_losses else None
        return dst, loss_out, tuple(np.frombuffer(raw[-8:], dtype=np.int32))
    return run


@pytest.mark.parametrize('K', J.SUM_K_CPU)
def test_host_build_is_numpys_left_to_right_float32_sum(host_program, K):
    """((a + b) + c) ... of NumPy float32, bit for bit: every n, the 16-byte path and the path of pointers one float off, dst of
    its own and dst aliasing the first and the last source; the loss slots likewise."""
    losses = J.loss_inputs(K)
    want_losses = J.numpy_losses(losses)
    seen = set()
    for n in J.SUM_N:
        srcs = J.sum_inputs(K, n)
        want = J.numpy_sum(srcs)
        if n >= 1025:                                # the inputs hold what they are said to hold, and no NaN arises from them
            assert np.isinf(srcs).any() and (srcs == 0).any() and ((np.abs(srcs) < 1.2e-38) & (srcs != 0)).any() and np.signbit(srcs[srcs == 0]).any()
            assert not np.isnan(want).any() and (K < 2 or (want == 0).any())
        for offset in (0, 1):
            for alias in sorted({-1, 0, K - 1}):
                dst, loss_out, (vec, blocks) = host_program(srcs, losses, offset=offset, alias=alias, tag='k%d_n%d' % (K, n))
                assert dst.tobytes() == want.tobytes(), (K, n, offset, alias, int((dst.view(np.uint32) != want.view(np.uint32)).sum()))
                assert loss_out.tobytes() == want_losses.tobytes(), (K, n, loss_out, want_losses)
                assert vec == (offset == 0) and blocks == max(1, -(-(n // 4 if vec else n) // 256))
                seen.add((vec, n % 4 != 0))
    assert seen == {(1, False), (1, True), (0, False), (0, True)}
    # without the losses: the same sum, and nothing is launched for nothing
    srcs = J.sum_inputs(K, 5)
    dst, loss_out, (vec, blocks) = host_program(srcs, losses, want_losses=False, tag='bare')
    assert loss_out is None and dst.tobytes() == J.numpy_sum(srcs).tobytes() and blocks == 1
    assert host_program(J.sum_inputs(K, 0), losses, want_losses=False, tag='nothing')[2][1] == 0


def test_the_order_of_the_additions_shows(host_program):
    """The cases tell left-to-right from any other order: a pairwise or right-to-left sum of the same inputs differs."""
    srcs = J.sum_inputs(3, 1025)
    want = J.numpy_sum(srcs)
    other = (srcs[0] + (srcs[1] + srcs[2])).astype(np.float32)
    assert (want.view(np.uint32) != other.view(np.uint32)).sum() >= 2 * (1025 // 11)
    v = J.loss_inputs(3)
    assert J.numpy_losses(v)[0] == 1.0 and np.float32(v[0] + np.float32(v[1] + v[2])) == 0.0
    assert host_program(srcs, v, tag='order')[1][0] == 1.0


def test_host_program_refuses_what_the_library_refuses(host_program):
    srcs, losses = J.sum_inputs(3, 8), J.loss_inputs(3)
    none = np.zeros((0, 0), dtype=np.float32)
    assert 'K must be' in host_program(none, losses[:0], K=0, n=8, status=1, tag='k0')
    assert 'K must be' in host_program(none, losses[:0], K=9, n=8, status=1, tag='k9')
    assert 'n must be' in host_program(none, losses[:0], K=3, n=-1, status=1, tag='neg')
    for bad, word in ((1, 'null src'), (2, 'null dst'), (3, 'src pointer not 4-byte'), (4, 'dst not 4-byte'), (5, 'null loss_in'),
                      (6, 'partially'), (7, 'loss_out overlaps')):
        assert word in host_program(srcs, losses, bad=bad, status=1, tag='bad%d' % bad), bad


def test_argument_validation_returns_before_any_device_call():
    """bhn_jnt_sum on a machine without a GPU: every refusal is BHN_EINVAL with a message, through pointers that are never
    dereferenced; n == 0 without losses succeeds without a launch."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    lib = _hip.jnt_lib()
    assert _hip.BHN_JNT_MAX_TERMS == J.MAX_TERMS == 8

    def ptrs(*addr):
        s = _hip.bhn_jnt_ptrs()
        for k, a in enumerate(addr):
            s.p[k] = a
        return s
    base = 1 << 20
    src3 = ptrs(base, 2 * base, 3 * base)
    loss3 = ptrs(4 * base, 4 * base + 4, 4 * base + 8)
    good = dict(src=C.byref(src3), K=3, n=1000, dst=C.c_void_p(5 * base), loss_in=C.byref(loss3), loss_out=C.c_void_p(6 * base))
    bad = [(dict(K=0), b'K must be'), (dict(K=-1), b'K must be'), (dict(K=9), b'K must be'), (dict(n=-1), b'n must be'),
           (dict(n=(1 << 40) + 1), b'n must be'), (dict(src=None), b'null src'), (dict(src=C.byref(ptrs(base, 0, 3 * base))), b'null src pointer'),
           (dict(src=C.byref(ptrs(base, 2 * base, 0))), b'null src pointer'), (dict(src=C.byref(ptrs(base, 2 * base, 0)), n=0), b'null src pointer'),
           (dict(dst=None), b'null dst'), (dict(src=C.byref(ptrs(base, 2 * base + 2, 3 * base))), b'src pointer not 4-byte'),
           (dict(dst=C.c_void_p(5 * base + 1)), b'dst not 4-byte'), (dict(loss_out=C.c_void_p(6 * base + 2)), b'loss_out not 4-byte'),
           (dict(loss_in=None), b'null loss_in'), (dict(loss_in=C.byref(ptrs(4 * base, 0, 4 * base + 8))), b'null loss_in pointer'),
           (dict(loss_in=C.byref(ptrs(4 * base, 4 * base + 4, 4 * base + 9))), b'loss_in pointer not 4-byte'),
           (dict(dst=C.c_void_p(base + 4)), b'partially'), (dict(dst=C.c_void_p(3 * base - 4)), b'partially'),
           (dict(dst=C.c_void_p(2 * base + 3996)), b'partially'), (dict(loss_out=C.c_void_p(5 * base + 3996)), b'loss_out overlaps')]
    for change, word in bad:
        a = dict(good, **change)
        rc = lib.bhn_jnt_sum(*[a[k] for k in good], None)
        assert rc == _hip.BHN_EINVAL, (change, rc, lib.bhn_jnt_last_error())
        msg = lib.bhn_jnt_last_error()
        assert msg and word in msg, (change, msg)
        with pytest.raises(_hip.HipError, match='libbhnerf_jnt'):
            _hip.jnt_check(rc)
    # nothing to do: no launch, no error -- whatever dst and the losses are
    assert lib.bhn_jnt_sum(C.byref(src3), 3, 0, None, None, None, None) == 0
    assert lib.bhn_jnt_sum(C.byref(src3), 3, 0, C.c_void_p(5 * base), C.byref(loss3), None, None) == 0
    _hip.jnt_check(0)
    # the Python wrappers refuse host tensors and wrong counts before the library is asked
    import torch
    from bhnerf_amd import engine
    with pytest.raises(_hip.HipError, match='device tensor'):
        engine.joint_sum([torch.zeros(4), torch.zeros(4)])
    with pytest.raises(AttributeError, match='1 to 8'):
        engine.joint_sum([])
    with pytest.raises(AttributeError, match='one size'):
        engine.joint_sum([torch.zeros(4), torch.zeros(5)])


JNT_NAMES = ['bhn_jnt_last_error', 'bhn_jnt_sum']


def test_jnt_library_exports_its_header_and_keeps_the_library_conventions():
    """libbhnerf_jnt.so: the dynamic symbol table is the declarations of include/bhnerf_jnt.h and nothing else, the ctypes table
    binds exactly those, the library references no allocator, no getenv and no synchronisation, and no other library, header or
    ctypes table knows a name that begins with bhn_jnt.  The eleventh library has a tuple of its own: _hip.LIBRARIES keeps its five
    keys."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    header = side._header('bhnerf_jnt.h')
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', header)))
    assert declared == sorted(_hip.JNT_SIGNATURES) == JNT_NAMES
    defined = side._symbols(_hip.JNT_LIB_PATH, '--defined-only')
    assert sorted(line.split()[-1] for line in defined.splitlines() if line.strip()) == declared
    undefined = side._symbols(_hip.JNT_LIB_PATH, '--undefined-only')
    for banned in side.BANNED:
        assert banned not in undefined, banned
    assert set(_hip.LIBRARIES) == {'libbhnerf_hip', 'libbhnerf_kerr', 'libbhnerf_eht', 'libbhnerf_grf', 'libbhnerf_eql'}
    assert _hip.JNT_LIBRARY == (_hip.JNT_LIB_PATH, _hip.JNT_SIGNATURES, 'bhn_jnt_last_error', None)
    assert len(_hip.JNT_LIBRARY) == len(_hip.REG_LIBRARY) and [type(v) for v in _hip.JNT_LIBRARY] == [type(v) for v in _hip.REG_LIBRARY]
    assert _hip.jnt_lib() is _hip.load(_hip.JNT_LIB_PATH, _hip.JNT_SIGNATURES)
    others = [('bhnerf_%s.h' % name.split('_')[1], path, table) for name, (path, table, _, _) in _hip.LIBRARIES.items()]
    others += [('bhnerf_%s.h' % n,) + getattr(_hip, n.upper() + '_LIBRARY')[:2] for n in ('flow', 'rec', 'cls', 'pol', 'reg')]
    assert len(others) == 10
    for other_header, path, table in others:
        assert 'bhn_jnt' not in side._header(other_header), other_header
        assert 'bhn_jnt' not in side._symbols(path, '--defined-only'), path
        assert not any(k.startswith('bhn_jnt') for k in table), other_header
    # the constants of the header are the binding's, and the struct is the header's: eight pointers by value
    assert int(re.search(r'#define BHN_JNT_MAX_TERMS (\d+)', header).group(1)) == _hip.BHN_JNT_MAX_TERMS
    assert int(re.search(r'#define BHN_JNT_MAX_BLOCKS (\d+)', header).group(1)) == _hip.BHN_JNT_MAX_BLOCKS
    assert C.sizeof(_hip.bhn_jnt_ptrs) == 8 * _hip.BHN_JNT_MAX_TERMS
    # the kernel's code stands on the shared skeleton and on nothing of another library
    src = open(os.path.join(side.ROOT, 'bhnerf_amd', 'csrc', 'joint_sum.hip')).read()
    assert '#include "side_lib.h"' in src and not re.search(r'atomic\w*\s*\(', src)
    assert sorted(re.findall(r'#include "([^"]+)"', src)) == ['../../include/bhnerf_jnt.h', 'joint_sum.h', 'side_lib.h']


def _steps():
    from bhnerf_amd import optimization
    T = optimization.TrainStep
    t = np.linspace(0.0, 1.0, 5)
    image = T.image(t, np.zeros((5, 4, 4)), scale=2.0, dtype='full')
    lc = T.image(t, np.zeros(5), scale=0.5, dtype='lc')
    uv = np.random.default_rng(0).normal(size=(5, 6, 2)) * 1e9
    vis = T.eht_uv(t, np.zeros((5, 6), dtype=np.complex64), np.ones((5, 6)), uv, 1e-10, 4, dtype='vis', scale=3.0)
    prior = T.volume_prior(20.0, resolution=4, weights={'tsv': 1.0}, scale=7.0)
    return T, t, image, lc, vis, prior


def test_joint_flattens_keeps_the_order_and_is_one_loss():
    from bhnerf_amd import network, optimization
    T, t, image, lc, vis, prior = _steps()
    j = T.joint(image, vis, prior)
    assert j.num_losses == 1 and list(j.dtype) == ['joint'] and list(j.scale) == [1.0]
    assert j.grad_pmap[0] is network.gradient_step_joint and j.test_pmap[0] is network.test_joint
    args = j.args[0]
    assert isinstance(args, optimization.JointArgs)
    assert [(kind, dtype, scale) for kind, dtype, _, scale in args.terms] == [('image', 'full', 2.0), ('eht', 'vis', 3.0), ('volume', 'volume', 7.0)]
    assert [a for _, _, a, _ in args.terms] == [image.args[0], vis.args[0], prior.args[0]]
    # sums and earlier joints are flattened in order
    nested = T.joint(prior + lc, T.joint(image, vis), lc)
    assert [(kind, dtype) for kind, dtype, _, _ in nested.args[0].terms] == [('volume', 'volume'), ('image', 'lc'), ('image', 'full'), ('eht', 'vis'),
                                                                             ('image', 'lc')]
    assert nested.num_losses == 1
    # a joint step is one term of a sum
    both = T.joint(image, prior) + vis
    assert both.num_losses == 2 and list(both.dtype) == ['joint', 'vis'] and list(both.scale) == [1.0, 3.0]
    assert both.grad_pmap[1] is network.gradient_step_eht and isinstance(both.args[0], optimization.JointArgs)
    assert T.joint(both).num_losses == 1 and len(T.joint(both).args[0].terms) == 3
    assert j.last_terms is None and image.last_terms is None and both.last_terms is None
    # at most eight terms, at least one, and only this class's step functions
    assert len(T.joint(*[image] * 8).args[0].terms) == 8
    with pytest.raises(ValueError, match='1 to 8'):
        T.joint(*[image] * 9)
    with pytest.raises(ValueError, match='1 to 8'):
        T.joint()
    foreign = T('full', image.args[0], lambda *a: None, lambda *a: None, 1.0)
    with pytest.raises(ValueError, match='terms of this class'):
        T.joint(image, foreign)
    assert 'eagerly' in T.joint.__doc__ and 'joint' in T.volume_prior.__doc__


def test_joint_needs_one_set_of_frame_times():
    from bhnerf_amd import units
    T, t, image, lc, vis, prior = _steps()
    other_values = T.image(t + 0.25, np.zeros((5, 4, 4)))
    fewer = T.image(t[:4], np.zeros((4, 4, 4)))
    minutes = T.image(t * units.hr, np.zeros((5, 4, 4)))
    minutes.args[0].t_frames = t * units.min                  # (TrainStep itself takes hours only: the unit is changed behind it)
    for bad in (other_values, fewer, minutes):
        with pytest.raises(ValueError, match='frame times|unit of time'):
            T.joint(image, bad)
        with pytest.raises(ValueError, match='frame times|unit of time'):
            T.joint(prior, bad, vis)
    with pytest.raises(ValueError, match='unit of time'):
        T.joint(image, minutes)
    assert T.joint(image, T.image(t * units.hr, np.zeros((5, 4, 4)))).num_losses == 1         # hours with and without the unit: one unit
    assert T.joint(prior, image, prior).args[0].num_frames == 5                              # priors carry no frame times


def test_joint_args_batch_the_terms_own_args():
    from bhnerf_amd import network, optimization, regularization, units
    T, t, image, lc, vis, prior = _steps()
    rng = np.random.default_rng(3)
    target = rng.normal(size=(5, 4, 4)).astype(np.float32)
    image = T.image(t, target, sigma=2.0, scale=2.0)
    args = T.joint(image, prior, vis).args[0]
    assert args.num_frames == 5 and units.unit_name(args.t_units) in ('hr', 'h') and args.t_start_obs == t[0]
    key = np.array([3, 1])
    targets, sigmas, thirds, t_frames = args[key]
    assert isinstance(targets, tuple) and isinstance(sigmas, tuple) and isinstance(thirds, network.JointOperands) and len(thirds) == 3
    np.testing.assert_array_equal(np.asarray(targets[0]), target[key])
    np.testing.assert_array_equal(np.asarray(sigmas[0]), np.full((2, 4, 4), 2.0, dtype=np.float32))
    np.testing.assert_array_equal(np.asarray(thirds[0]), np.zeros((2, 4, 4), dtype=np.float32))
    assert targets[1] is None and sigmas[1] is None and isinstance(thirds[1], regularization.VolumePrior) and thirds[1] is prior.args[0].op
    assert np.asarray(targets[2]).shape == (2, 6) and thirds[2].shape[0] == 2
    np.testing.assert_array_equal(t_frames, t[key])
    assert thirds.terms == (('image', 'full', 2.0), ('volume', 'volume', 7.0), ('eht', 'vis', 3.0)) and thirds.owner is args
    # sampling is the first frame-bearing term's: the same draws as that term alone
    twin = T.image(t, target)
    draws = [args.sample(2) for _ in range(3)]
    assert [d.tolist() for d in draws] == [twin.args[0].sample(2).tolist() for _ in range(3)] and all(len(set(d)) == 2 for d in draws)
    # priors only: StaticArgs' behaviour
    alone = T.joint(prior, prior).args[0]
    static = optimization.StaticArgs(prior.args[0].op)
    assert alone.num_frames == static.num_frames == 1 and alone.t_units == static.t_units
    assert alone.sample(5).tolist() == static.sample(5).tolist() == [0] * 5
    got = alone[np.array([4, 2])]
    assert got[0] == (None, None) and got[1] == (None, None) and got[2][0] is got[2][1] is prior.args[0].op
    np.testing.assert_array_equal(got[3], static[0][3])
    # the step functions refuse what is not a joint call, before the device is needed
    with pytest.raises(AttributeError, match='JointOperands'):
        network.gradient_step_joint(None, None, 'joint', (None,), (None,), (prior.args[0].op,), *([None] * 10), 1.0)
    with pytest.raises(AttributeError, match='joint dtype'):
        network.test_joint(None, None, 'full', got[0], got[1], got[2], *([None] * 10), 1.0)
    with pytest.raises(AttributeError, match='scale 1'):
        network.test_joint(None, None, 'joint', got[0], got[1], got[2], *([None] * 10), 2.0)
    with pytest.raises(AttributeError, match='kind'):
        network.JointOperands([None], [('pixels', 'full', 1.0)])
    with pytest.raises(AttributeError, match='not supported'):
        network.test_joint(None, None, 'joint', (None,), (None,), network.JointOperands([None], [('image', 'vis', 1.0)]), *([None] * 10), 1.0)
