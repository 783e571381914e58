"""GPU tests of the joint training step (optimization.TrainStep.joint, network.gradient_step_joint) and of its fan-in kernel
(libbhnerf_jnt.so, csrc/joint_sum.hip).

Every comparison is bitwise.  The kernel is held to NumPy's float32 left-to-right sum (tests/joint_cases.py), the step to a
hand-built sequence of the same launches with torch's `+` in the place of the kernel: a float32 sum in a given order has one
correct answer, so there is no tolerance here.  The problem: a 4x128 network (posenc_deg 3) on 8 x 8 rays x 16 samples, 4 frames in
batches of 2, a prior lattice of 8^3, 6 baselines of 4 stations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_cases as J                                                # noqa: E402
from gpu_support import Out, dev, stream_ptr                           # noqa: E402,F401

SENTINEL = -777.0
_INPUTS = {}


def inputs_of(K, n):
    """(the K vectors, their NumPy sum), computed once and shared."""
    if (K, n) not in _INPUTS:
        srcs = J.sum_inputs(K, n)
        _INPUTS[K, n] = (srcs, J.numpy_sum(srcs))
    return _INPUTS[K, n]


def _ptrs(addresses):
    from bhnerf_amd import _hip
    s = _hip.bhn_jnt_ptrs()
    for k, a in enumerate(addresses):
        s.p[k] = a
    return s


def _device_sum(dev, srcs, shift, alias, losses=None):
    """bhn_jnt_sum on vectors that start `shift` floats behind a 16-byte boundary, each between two guard bands; dst of its own or
    (alias k) src[k] itself -> (dst, loss_out or None) as NumPy arrays; the guards and the sources that are not dst are checked."""
    from bhnerf_amd import _hip
    K, n = srcs.shape
    pad = 1 if n == 0 else 0                                         # (an empty tensor has no address: one element that the call must leave alone)
    held = [np.concatenate([srcs[k], np.full(pad, 5.0, dtype=np.float32)]) for k in range(K)]
    bufs = [Out(n + pad, dev, shift=shift, init=held[k], guard=64, sentinel=SENTINEL) for k in range(K)]
    dst = bufs[alias] if alias >= 0 else Out(n + pad, dev, shift=shift, guard=64, sentinel=SENTINEL)
    src = _ptrs([b.view.data_ptr() for b in bufs])
    lin = lout = None
    if losses is not None:
        lin = torch.as_tensor(losses, device=dev)
        lout = Out(K + 1, dev, guard=64, sentinel=SENTINEL)
    rc = _hip.jnt_lib().bhn_jnt_sum(C.byref(src), K, n, dst.view.data_ptr(), None if lin is None else C.byref(_ptrs([lin.data_ptr() + 4 * k for k in range(K)])),
                                    None if lout is None else lout.view.data_ptr(), stream_ptr(dev))
    _hip.jnt_check(rc)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        got = b.numpy()                                              # (asserts the bytes on either side)
        if b is not dst:
            assert got.tobytes() == held[k].tobytes(), 'a source was written'
    out = dst.numpy()
    assert pad == 0 or out[n] == (5.0 if alias >= 0 else SENTINEL), 'an element beyond n was written'
    return out[:n], (None if lout is None else lout.numpy())


@pytest.mark.parametrize('shift', (0, 1))
@pytest.mark.parametrize('K', J.SUM_K_GPU)
def test_device_sum_is_numpys_left_to_right_float32_sum(dev, K, shift):
    """Every n of the CPU test and n = BHN_JNT_MAX_BLOCKS 1024 + 5 (a second trip of the grid-stride loop on the 16-byte path, a
    fifth on the other), 16-byte aligned pointers and pointers one float off, dst of its own and in place on the first and the
    last source; the loss slots; the bytes on either side of every vector are unchanged."""
    from bhnerf_amd import _hip
    big = _hip.BHN_JNT_MAX_BLOCKS * 1024 + 5
    losses = J.loss_inputs(K)
    for n in J.SUM_N + (big,):
        srcs, want = inputs_of(K, n)
        for alias in sorted({-1, 0, K - 1}):
            dst, lout = _device_sum(dev, srcs, shift, alias, losses=losses if alias < 0 else None)
            diff = int((dst.view(np.uint32) != want.view(np.uint32)).sum())
            assert diff == 0, (K, n, shift, alias, diff)
            if lout is not None:
                assert lout.tobytes() == J.numpy_losses(losses).tobytes(), (K, n, lout)


def test_device_sum_edges_and_refusals(dev):
    from bhnerf_amd import _hip, engine
    lib = _hip.jnt_lib()
    srcs, want = inputs_of(3, 1025)
    # a partial overlap is refused before any launch: nothing is written
    bufs = [Out(1025, dev, init=srcs[k], guard=64, sentinel=SENTINEL) for k in range(3)]
    src = _ptrs([b.view.data_ptr() for b in bufs])
    for shifted in (bufs[0].view.data_ptr() + 4, bufs[2].view.data_ptr() - 4, bufs[1].view.data_ptr() + 4 * 1024):
        assert lib.bhn_jnt_sum(C.byref(src), 3, 1025, shifted, None, None, stream_ptr(dev)) == _hip.BHN_EINVAL
        assert b'partially' in lib.bhn_jnt_last_error()
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        assert b.numpy().tobytes() == srcs[k].tobytes()
    # losses only (n = 0), the loss pointers pointing into loss_out itself: the K values are read before anything is written
    v = J.loss_inputs(3)
    lout = Out(4, dev, init=np.concatenate([[0.0], v]).astype(np.float32), guard=64, sentinel=SENTINEL)
    inside = _ptrs([lout.view.data_ptr() + 4 * (1 + k) for k in range(3)])
    _hip.jnt_check(lib.bhn_jnt_sum(C.byref(inside), 3, 0, None, C.byref(inside), lout.view.data_ptr(), stream_ptr(dev)))
    torch.cuda.synchronize()
    assert lout.numpy().tobytes() == J.numpy_losses(v).tobytes()
    # the Python wrappers: a slice such as buf[1:] takes the element path, out may be a part, the losses come as K + 1 floats
    parts = [torch.as_tensor(srcs[k], device=dev) for k in range(3)]
    assert engine.joint_sum(parts).cpu().numpy().tobytes() == want.tobytes()
    sliced = [p[1:] for p in parts]
    assert sliced[0].data_ptr() % 16 == 4 and engine.joint_sum(sliced).cpu().numpy().tobytes() == J.numpy_sum(srcs[:, 1:]).tobytes()
    out = engine.joint_sum(parts, out=parts[0])
    assert out is parts[0] and out.cpu().numpy().tobytes() == want.tobytes()
    lv = engine.joint_losses([torch.as_tensor(v[k:k + 1], device=dev) for k in range(3)])
    assert lv.shape == (4,) and lv.cpu().numpy().tobytes() == J.numpy_losses(v).tobytes()
    with pytest.raises(AttributeError, match='contiguous float32'):
        engine.joint_sum([parts[1][::2], parts[2][::2]])


# ---- the step --------------------------------------------------------------------------------------------------------------
def _hand_step(state, pred, rt, idx, terms):
    """One joint step written out: pack -> render_train (render without a tape) -> each ray term's engine.chi2_* -> torch's
    d_0 + d_1 -> render_bwd_tape (render_bwd) into the gradient buffer -> each prior's lattice pass into a buffer of its own ->
    torch's g_0 + g_1 -> apply_gradients.  Returns (total loss, [term losses]); the operands are the terms' own args at `idx`."""
    from bhnerf_amd import engine, network, units
    eng = pred.engine()
    n = eng.nparams
    buf = state.grad_buffer()
    eng.pack(state.flat)
    ray = [t for t in terms if str(t.dtype[0]) != 'volume']
    losses, parts = {}, []
    if ray:
        geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], network._stokes_or_none(rt['J']), rt['g'], rt['dtau'], rt['Sigma'])
        tM0, _ = network._frame_offsets(ray[0].args[0][idx][3], units.hr, rt['t_start_obs'], rt['t_injection'], eng.device)
        B = int(tM0.numel())
        taped = eng.fits_tape(B, geom.P_eff)
        images = (eng.render_train if taped else eng.render)(geom, tM0)
        d = None
        for t in ray:
            target, sigma, third, _ = t.args[0][idx]
            dtype, scale = str(t.dtype[0]), float(t.scale[0])
            if t.grad_pmap[0] is network.gradient_step_image:
                loss, dk = engine.chi2_image(images, *network._image_operands(geom, B, dtype, (target, sigma, third), eng.device), scale, dtype)
            else:
                loss, dk = engine.chi2_eht(images, third, target, sigma, scale, dtype)
            losses[id(t)] = loss
            d = dk if d is None else d + dk
        (eng.render_bwd_tape if taped else eng.render_bwd)(geom, tM0, d, out=buf[:n])
        parts.append(buf[:n])
    for t in terms:
        if str(t.dtype[0]) != 'volume':
            continue
        op = t.args[0].op
        geom = pred.geometry(op.coords, 0.0, 0.0)
        tM0, _ = network._frame_offsets(np.array([0.0]), units.hr, rt['t_start_obs'], 0.0, eng.device)
        taped = eng.fits_tape(1, geom.P_eff)
        volume = (eng.render_train if taped else eng.render)(geom, tM0)
        loss, dv = engine.chi2_volume(volume, op, float(t.scale[0]), mask=geom.dom)
        losses[id(t)] = loss.clone()
        grad = buf[:n] if not parts else torch.empty((n,), dtype=torch.float32, device=eng.device)
        (eng.render_bwd_tape if taped else eng.render_bwd)(geom, tM0, dv, out=grad)
        parts.append(grad)
    total = parts[0]
    for g in parts[1:]:
        total = total + g
    if len(parts) > 1:
        buf[:n].copy_(total)
    state.apply_gradients(buf[:n])
    each = [losses[id(t)] for t in terms]
    loss = each[0].clone()
    for x in each[1:]:
        loss = loss + x
    return loss, torch.cat(each)


BATCHES = (np.array([2, 0]), np.array([1, 3]), np.array([3, 2]))


def _compare_three_steps(dev, mode, terms, stokes=False):
    from bhnerf_amd import optimization
    pred, flat0 = J.predictor(mode, dev)
    rt = J.ray_set(stokes)
    step = optimization.TrainStep.joint(*terms)
    state, hand = J.new_state(pred, flat0, rt), J.new_state(pred, flat0, rt)
    assert step.last_terms is None
    for i, idx in enumerate(BATCHES):
        loss, state, images = step(state, rt, idx)
        hloss, hterms = _hand_step(hand, pred, rt, idx, terms)
        assert state.step == hand.step == i + 1
        assert torch.equal(state.flat, hand.flat) and torch.equal(state.m, hand.m) and torch.equal(state.v, hand.v), (mode, i)
        assert loss.shape == (1,) and torch.equal(loss, hloss) and bool(torch.isfinite(loss).all()) and float(loss) > 0
        assert step.last_terms.shape == (len(terms),) and torch.equal(step.last_terms, hterms) and bool((hterms > 0).all())
        assert images.shape == (1, J.BATCH) + ((3,) if stokes else ()) + (J.H, J.W)
    assert float((state.flat - flat0).abs().max()) > 0 and float(state.grad[:pred.engine().nparams].abs().max()) > 0
    return pred, rt


@pytest.mark.parametrize('mode', ('f32', 'bf16'))
def test_joint_step_is_the_hand_built_step(dev, mode):
    """image('full') + eht_uv('vis') + volume_prior({'tv': 1}) as ONE step: parameters, m, v, the returned loss and last_terms over
    three consecutive steps are bitwise those of the sequence written out in _hand_step."""
    pred, rt = _compare_three_steps(dev, mode, J.data_terms())
    geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], None, rt['g'], rt['dtau'], rt['Sigma'])
    assert pred.engine().fits_tape(J.BATCH, geom.P_eff)              # the taped path ran


def test_joint_step_without_a_tape_is_the_hand_built_step(dev, monkeypatch):
    """fits_tape False on both sides: render + render_bwd for the ray group and for the lattice."""
    from bhnerf_amd import engine
    monkeypatch.setattr(engine.FusedPredictor, 'fits_tape', lambda self, B, P: False)
    _compare_three_steps(dev, 'bf16', J.data_terms())


def test_joint_step_on_stokes_rays_is_the_hand_built_step(dev):
    """eht_closure('cphase+logcamp') + eht_pol('m') on three Stokes planes, the combination of the station-gain example: one render,
    the two d loss / d images added, one backward, one Adam step."""
    _compare_three_steps(dev, 'bf16', J.stokes_terms(), stokes=True)


def _run(dev, step, steps=2, mode='bf16'):
    pred, flat0 = J.predictor(mode, dev)
    rt = J.ray_set()
    state = J.new_state(pred, flat0, rt)
    for idx in BATCHES[:steps]:
        _, state, _ = step(state, rt, idx)
    return state


def test_a_zero_weight_term_changes_nothing_in_a_joint_step_and_does_in_a_sum(dev):
    """joint(image, prior of scale 0) is the image-only step, bit for bit; image + prior of scale 0 is not: the prior's Adam step
    on a zero gradient still moves the parameters through the moments it shares with the data term.  The reason joint exists."""
    from bhnerf_amd.optimization import TrainStep
    image, _, _ = J.data_terms()
    zero = TrainStep.volume_prior(J.FOV_M, resolution=J.RES, weights={'tv': 1.0}, eps=1e-4, scale=0.0)
    alone = _run(dev, image)
    joint = _run(dev, TrainStep.joint(image, zero))
    summed = _run(dev, image + zero)
    assert alone.step == joint.step == 2 and summed.step == 4
    for name in ('flat', 'm', 'v'):
        assert torch.equal(getattr(joint, name), getattr(alone, name)), name
    assert not torch.equal(summed.flat, alone.flat) and not torch.equal(summed.m, alone.m) and not torch.equal(summed.v, alone.v)


def test_test_mode_sums_the_terms_own_test_losses_and_touches_nothing(dev):
    from bhnerf_amd import optimization
    terms = J.data_terms()
    step = optimization.TrainStep.joint(*terms)
    pred, flat0 = J.predictor('bf16', dev)
    rt = J.ray_set()
    state = J.new_state(pred, flat0, rt)
    state.m.fill_(0.25); state.v.fill_(0.5)
    grad0 = state.grad.clone()
    idx = BATCHES[0]
    own = [t(state, rt, idx, update_state=False) for t in terms]
    want = (own[0][0] + own[1][0]) + own[2][0]
    loss, out_state, images = step(state, rt, idx, update_state=False)
    assert out_state is state and state.step == 0 and torch.equal(state.flat, flat0) and torch.equal(state.grad, grad0)
    assert bool((state.m == 0.25).all()) and bool((state.v == 0.5).all())
    assert torch.equal(loss, want) and torch.equal(step.last_terms, torch.cat([o[0] for o in own]))
    assert torch.equal(images, own[0][2]) and images.shape == (1, J.BATCH, J.H, J.W)
    # priors only: the prior's loss, a 0-d zero for the images
    alone = optimization.TrainStep.joint(terms[2])
    loss, _, images = alone(state, rt, alone.args[0].sample(J.BATCH), update_state=False)
    assert torch.equal(loss, own[2][0]) and images.ndim == 0 and float(images) == 0.0
    # the whole movie: the same sum accumulated per chunk of BATCH frames (the prior counts once per chunk)
    total = 0.0
    for chunk in optimization._movie_chunks(J.NT, J.BATCH, 1):
        parts = [t(state, rt, chunk, update_state=False)[0] for t in terms]
        total = total + ((parts[0] + parts[1]) + parts[2]).sum()
    assert optimization.total_movie_loss(J.BATCH, state, step, rt) == float(total) / J.NT
    assert state.step == 0 and torch.equal(state.flat, flat0)


def test_optimizer_run_with_a_joint_step_is_the_manual_loop(dev):
    from bhnerf_amd import optimization
    terms = J.data_terms()
    pred, flat0 = J.predictor('bf16', dev)
    rt = J.ray_set()
    opt = optimization.Optimizer(dict(J.HP, num_iters=3), pred, rt)
    with torch.no_grad():
        opt.state.flat.copy_(flat0)
    step = optimization.TrainStep.joint(*terms)
    twin = optimization.TrainStep.image(J.t_frames(), np.zeros((J.NT, J.H, J.W)))            # the same draws as the joint's first term
    batches = [twin.args[0].sample(J.BATCH) for _ in range(3)]
    opt.run(J.BATCH, step, rt)
    hand = optimization.Optimizer(dict(J.HP, num_iters=3), pred, rt).state
    with torch.no_grad():
        hand.flat.copy_(flat0)
    for idx in batches:
        hloss, hterms = _hand_step(hand, pred, rt, idx, terms)
    assert opt.state.step == hand.step == 3
    assert torch.equal(opt.state.flat, hand.flat) and torch.equal(opt.state.m, hand.m) and torch.equal(opt.state.v, hand.v)
    assert np.isfinite(np.log10(np.mean(opt.loss))) and float(np.mean(opt.loss)) == float(hloss) and torch.equal(step.last_terms, hterms)
