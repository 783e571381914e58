"""GPU tests of the volume priors (libbhnerf_reg.so, csrc/vol_reg.hip) and of the training step on them
(network.gradient_step_volume, optimization.TrainStep.volume_prior).

Bound: the project's f32 bound, eht_uv_cases.F32_TOL = 2e-5, against the float64 autograd reference of tests/vol_reg_cases.py: the
loss slots and the per_volume sums relative, the gradient relative to its largest element.  The figures of every case are printed.
MEASURED_WORST records the worst values of a run on one MI355X (also DESIGN.md 4.18)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402
import vol_reg_cases as R                                              # noqa: E402
from guarded import Guarded                                            # noqa: E402
from gpu_support import dev                                           # noqa: E402,F401
from mlp_bounds import IMG_TOL                                         # noqa: E402

TOL = E.F32_TOL
MEASURED_WORST = {'loss': 1.39e-7, 'per_volume': 1.14e-7, 'gradient': 1.62e-7}        # smooth hotspot, 1x1x5, 66x64x64
_REFS = {}


def ref_of(name):
    """The float64 reference of a case, computed once and shared."""
    if name not in _REFS:
        c = R.make_case(name)
        _REFS[name] = (c, R.reference(c['e'], c['mask'], c['spacing'], c['weights'], c['eps'], c['scale']))
    return _REFS[name]


def _f3(v):
    return (C.c_float * 3)(*v)


def _raw(c, dev):
    """The case on the device and call(loss, per_volume, dvolumes, ws, ws_bytes, **changes) -> the return code of bhn_reg_loss."""
    from bhnerf_amd import _hip
    lib = _hip.reg_lib()
    e = torch.as_tensor(np.ascontiguousarray(c['e']), device=dev)
    mask = None if c['mask'] is None else torch.as_tensor(np.ascontiguousarray(c['mask']), device=dev)
    N, dims = int(e.shape[0]), tuple(int(n) for n in e.shape[1:])
    need = int(lib.bhn_reg_ws_bytes(N, *dims))

    def call(loss, per_volume, dvolumes, ws, ws_bytes, **kw):
        a = dict(dict(c, e=e, mask=mask, N=N), **kw)
        return lib.bhn_reg_loss(a['e'].data_ptr(), a['N'], *dims, None if a['mask'] is None else a['mask'].data_ptr(), _f3(a['spacing']),
                                _f3(a['weights']), a['eps'], a['scale'], loss, per_volume, dvolumes, ws, ws_bytes, _hip.stream_ptr(dev))
    return dict(e=e, mask=mask, N=N, dims=dims, need=need, call=call)


def _run(c, dev, want_grad=True, **kw):
    """bhn_reg_loss on fresh buffers -> (loss[4], per_volume (3, N), dvolumes or None) as device tensors."""
    from bhnerf_amd import _hip
    r = _raw(c, dev)
    N = kw.get('N', r['N'])
    e = kw.get('e', r['e'])
    loss = torch.full((4,), float('nan'), device=dev)
    pv = torch.full((3, N), float('nan'), device=dev)
    dvol = torch.full((N,) + r['dims'], float('nan'), device=dev) if want_grad else None
    need = int(_hip.reg_lib().bhn_reg_ws_bytes(N, *r['dims']))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    assert e.shape[0] == N
    _hip.reg_check(r['call'](loss.data_ptr(), pv.data_ptr(), dvol.data_ptr() if want_grad else None, ws.data_ptr(), need, **kw))
    return loss, pv, dvol


@pytest.mark.parametrize('name', R.ALL_CASES)
def test_parity_with_float64(dev, name):
    c, (loss_ref, pv_ref, grad_ref) = ref_of(name)
    loss, pv, dvol = _run(c, dev)
    loss, pv, grad = loss.cpu().numpy(), pv.cpu().numpy(), dvol.cpu().numpy()
    assert np.isfinite(loss).all() and np.isfinite(pv).all() and np.isfinite(grad).all()
    le, pe, ge = R.loss_error(loss, loss_ref), R.loss_error(pv, pv_ref), R.grad_error(grad, grad_ref)
    print('%s: loss %.2e per_volume %.2e gradient %.2e' % (name, le, pe, ge))
    assert le < TOL and pe < TOL and ge < TOL
    if c['mask'] is not None:
        assert not grad[:, c['mask'] == 0].any()                     # exactly 0 outside the mask
    # forward only: the same loss, bit for bit
    assert torch.equal(_run(c, dev, want_grad=False)[0].cpu(), torch.from_numpy(loss))


def test_engine_call_is_the_library_call(dev):
    """engine.chi2_volume hands the operator's lattice, weights and eps to bhn_reg_loss: the same bits as the raw call; normalised,
    the weights are divided by the in-domain voxels; a host mask and a (nx, ny, nz) volume are taken too."""
    from bhnerf_amd import engine, regularization
    c = R.smooth_case(1e-3)
    axes = [np.linspace(-h, h, n) for h, n in zip((10.0, 10.0, 4.0), c['e'].shape[1:])]
    coords = np.array(np.meshgrid(*axes, indexing='ij'))
    names = dict(zip(R.TERMS, c['weights']))
    op = regularization.VolumePrior(coords=coords, weights=names, eps=c['eps'], normalize=False)
    c32 = dict(c, spacing=tuple(np.float32(op.spacing)))
    e = torch.as_tensor(c['e'], device=dev)
    loss, dvol = engine.chi2_volume(e, op, c['scale'], mask=c['mask'])
    raw = _run(c32, dev)
    assert loss.shape == (1,) and dvol.shape == e.shape and torch.equal(op.last_terms, raw[0]) and torch.equal(dvol, raw[2])
    assert torch.equal(op.last_per_volume, raw[1]) and torch.equal(loss, raw[0][:1])
    assert engine.chi2_volume(e[0], op, c['scale'], mask=torch.as_tensor(c['mask'], device=dev), want_grad=False)[1] is None
    assert torch.equal(op.last_terms, raw[0])
    count = int(c['mask'].sum())
    mean = regularization.VolumePrior(coords=coords, weights=names, eps=c['eps'])
    engine.chi2_volume(e, mean, c['scale'], mask=c['mask'])
    want = _run(dict(c32, weights=tuple(w / count for w in c['weights'])), dev)[0]
    assert torch.equal(mean.last_terms, want) and abs(float(want[0]) * count / float(raw[0][0]) - 1) < 1e-5


def test_bitwise_reproducible_and_independent_of_the_batch(dev):
    c = R.make_case('33x17x9')                                   # five workgroups per volume
    rng = np.random.default_rng(11)
    vols = (rng.uniform(0, 1, (3,) + c['e'].shape[1:]).astype(np.float32) * c['mask'])
    put = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    first = _run(c, dev, e=put(vols), N=3)
    again = _run(c, dev, e=put(vols), N=3)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    alone = [_run(c, dev, e=put(vols[i:i + 1]), N=1) for i in range(3)]
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (1, 2, 0)):
        loss, pv, dvol = _run(c, dev, e=put(vols[list(order)]), N=3)
        for slot, i in enumerate(order):
            assert torch.equal(dvol[slot], alone[i][2][0]) and torch.equal(pv[:, slot], alone[i][1][:, 0]), (order, slot)
    assert float(first[2].abs().max()) > 0


GUARD = 4096          # bytes on either side of a buffer: 0xA5 there, the buffer itself poisoned with NaN bytes (0xFF)


@pytest.mark.parametrize('name', ('1x1x1', '13x7x11', '33x17x9', 'no_mask', '64x64x64'))
def test_buffer_contract(dev, name):
    from bhnerf_amd import _hip
    c, (loss_ref, pv_ref, grad_ref) = ref_of(name)
    r = _raw(c, dev)
    N, need, call = r['N'], r['need'], r['call']
    V = int(np.prod(r['dims']))
    mk = lambda label, nbytes: Guarded(label, nbytes, 0xFF, dev, guard=GUARD, guard_fill=0xA5)
    loss, pv, dvol, ws = mk('loss', 16), mk('per_volume', 12 * N), mk('dvolumes', 4 * N * V), mk('ws', need)
    bufs = (loss, pv, dvol, ws)
    intact = lambda: all(b.disturbed() is None for b in bufs)
    # one byte too little workspace, a bad eps: refused, nothing launched
    assert call(loss.ptr, pv.ptr, dvol.ptr, ws.ptr, need - 1) == _hip.BHN_EWORKSPACE
    assert call(loss.ptr, pv.ptr, dvol.ptr, ws.ptr, need, eps=0.0) == _hip.BHN_EINVAL
    assert b'eps' in _hip.reg_lib().bhn_reg_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)
    # forward only: no gradient is written; per_volume NULL: the loss alone
    assert call(loss.ptr, None, None, ws.ptr, need) == 0
    torch.cuda.synchronize()
    four = loss.f32().copy()
    assert dvol.untouched() and pv.untouched() and np.isfinite(four).all() and intact()
    assert R.loss_error(four, loss_ref) < TOL
    # everything, into poisoned buffers of exactly the documented sizes
    loss.mid.fill_(0xFF); ws.mid.fill_(0xFF)
    assert call(loss.ptr, pv.ptr, dvol.ptr, ws.ptr, need) == 0
    torch.cuda.synchronize()
    assert intact()
    assert loss.poisoned(4) == 0 and pv.poisoned(4) == 0 and dvol.poisoned(4) == 0           # every element written
    assert loss.f32().tobytes() == four.tobytes()
    assert R.loss_error(pv.f32().reshape(3, N), pv_ref) < TOL and R.grad_error(dvol.f32().reshape(grad_ref.shape), grad_ref) < TOL


def test_absent_terms_masked_voxels_and_masked_contents(dev):
    c = R.make_case('13x7x11')
    full = _run(c, dev)
    for weights in R.SINGLE_WEIGHTS:
        d = weights.index(1.0)
        loss, pv, dvol = _run(dict(c, weights=weights, eps=c['eps'] if d == 0 else 0.0), dev)      # no tv: no requirement on eps
        for other in set(range(3)) - {d}:
            assert float(loss[1 + other]) == 0.0 and not bool(pv[other].any())
        assert torch.equal(pv[d], full[1][d]) and float(loss[0]) == float(loss[1 + d]) and bool(torch.isfinite(dvol).all())
    # a weight set to 0 leaves the other slots' bits as they are
    for d in range(3):
        w = tuple(0.0 if i == d else v for i, v in enumerate(c['weights']))
        loss, pv, dvol = _run(dict(c, weights=w), dev)
        assert float(loss[1 + d]) == 0.0
        for other in set(range(3)) - {d}:
            assert torch.equal(loss[1 + other], full[0][1 + other]) and torch.equal(pv[other], full[1][other])
    out = torch.as_tensor(c['mask'] == 0, device=dev)
    assert not bool(full[2][:, out].any()) and bool(full[2][:, ~out].any())
    junk = torch.as_tensor(c['e'], device=dev).clone()
    junk[:, out] = torch.tensor([float('nan'), float('inf'), -3e38, 7.0], device=dev)[torch.arange(int(out.sum()), device=dev) % 4]
    for a, b in zip(full, _run(c, dev, e=junk)):
        assert torch.equal(a, b)
    zero = _run(dict(c, weights=(0.0, 0.0, 0.0), eps=float('nan')), dev)
    assert not any(bool(t.any()) for t in zero)


# ---- the training step -----------------------------------------------------------------------------------------------------
def _ray_set():
    from bhnerf_amd import network, synthetic, units
    geo = synthetic.synthetic_geodesics(8, 8, 24, fov_M=16.0, seed=3)
    return network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                        t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr)


def _predictor(kind, dev):
    """(predictor, initial flat parameters, lattice resolution): a 4x128 NeRF in f32 or bf16 at 16^3, a voxel grid at 12^3; the
    domain 2 <= r <= 8, |z| <= 4 cuts the lattice of fov 16."""
    from bhnerf_amd import network
    rng = np.random.default_rng(5)
    if kind == 'grid':
        pred = network.GRID_Predictor(8.0, 2.0, 8.0, 4.0, grid_res=12, device=dev)
        flat = pred.init_params().flat.clone()
        flat += torch.as_tensor(rng.normal(6.0, 2.0, flat.numel()).astype(np.float32), device=dev)
        return pred, flat, 12
    pred = network.NeRF_Predictor(8.0, 2.0, 8.0, 4.0, net_depth=4, net_width=128, mode=kind, device=dev)
    params = pred.init_params(seed=3)
    with torch.no_grad():                                  # emission sigmoid(out - 10): a large bias makes the volume visible
        pred.engine().unflatten(params.flat)['MLP_0']['Dense_4']['bias'] += 8.0
    return pred, params.flat.clone(), 16


HP = {'num_iters': 10, 'lr_init': 1e-3, 'lr_final': 1e-5, 'seed': 3}


def _state(pred, flat, rt):
    from bhnerf_amd import optimization
    opt = optimization.Optimizer(HP, pred, rt)
    with torch.no_grad():
        opt.state.flat.copy_(flat)
    return opt.state


@pytest.mark.parametrize('kind', ('f32', 'bf16', 'grid'))
def test_one_training_step_is_the_hand_built_step(dev, kind):
    """TrainStep.volume_prior: loss, gradient and parameters are bitwise those of pack -> lattice geometry -> render_train ->
    bhn_reg_loss -> render_bwd_tape -> Adam written out here; test mode returns the same loss and steps nothing; last_volume is
    what sample_3d_grid gives on the lattice."""
    from bhnerf_amd import _hip, network, optimization, units
    pred, flat0, res = _predictor(kind, dev)
    rt = _ray_set()
    weights, eps, scale, fov = {'tv': 1.0, 'tsv': 0.05, 'l1': 0.3}, 1e-4, 2.5, 16.0
    step = optimization.TrainStep.volume_prior(fov, resolution=res, weights=weights, eps=eps, scale=scale)
    op = step.args[0].op
    state = _state(pred, flat0, rt)
    idx = step.args[0].sample(4)
    test_loss, _, test_imgs = step(state, rt, idx, update_state=False)
    assert state.step == 0 and torch.equal(state.flat, flat0) and test_imgs.ndim == 0 and float(test_imgs) == 0.0
    volume = op.last_volume.clone()
    loss, state, imgs = step(state, rt, idx)
    assert imgs.ndim == 0 and float(imgs) == 0.0 and state.step == 1 and float((state.flat - flat0).abs().max()) > 0
    assert float(loss.sum()) == float(test_loss.sum()) and np.isfinite(float(loss.sum())) and float(loss.sum()) > 0
    assert torch.equal(op.last_volume, volume) and volume.shape == (res,) * 3 and float(op.last_terms[0]) == float(loss.sum())
    # the same step by hand
    hand = _state(pred, flat0, rt)
    eng = pred.engine()
    geom = pred.geometry(op.coords, 0.0, 0.0)
    inside = int(geom.dom.sum())
    assert geom.G == 1 and geom.R == res ** 3 and 0 < inside < res ** 3
    tM0, _ = network._frame_offsets(np.array([0.0]), units.hr, rt['t_start_obs'], 0.0, eng.device)
    eng.pack(hand.flat)
    assert eng.fits_tape(1, geom.P_eff)
    images = eng.render_train(geom, tM0)
    assert images.shape == (1, 1, res ** 3) and torch.equal(images.reshape(volume.shape), volume)
    lib = _hip.reg_lib()
    need = int(lib.bhn_reg_ws_bytes(1, res, res, res))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    hloss = torch.empty((4,), dtype=torch.float32, device=dev)
    dvol = torch.empty_like(images)
    w = tuple(weights[k] / inside for k in R.TERMS)
    _hip.reg_check(lib.bhn_reg_loss(images.data_ptr(), 1, res, res, res, geom.dom.data_ptr(), _f3(op.spacing), _f3(w), eps, scale, hloss.data_ptr(),
                                    None, dvol.data_ptr(), ws.data_ptr(), need, _hip.stream_ptr(dev)))
    n = eng.nparams
    buf = hand.grad_buffer()
    eng.render_bwd_tape(geom, tM0, dvol, out=buf[:n])
    hand.apply_gradients(buf[:n])
    assert float(loss.sum()) == float(hloss[0]) and torch.equal(op.last_terms, hloss)
    assert torch.equal(state.grad[:n], hand.grad[:n]) and float(state.grad[:n].abs().max()) > 0
    assert torch.equal(state.flat, hand.flat)
    # the sampled volume against sample_3d_grid on the same lattice (the parameters before the step)
    mode = 'f32' if kind == 'grid' else kind
    ref = network.sample_3d_grid(pred.apply, _tree(eng, flat0), fov=fov, resolution=res)
    got = volume.cpu().numpy()
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print('%s: last_volume against sample_3d_grid %.2e of the largest voxel, bitwise %s' % (kind, err, bool((got == ref).all())))
    assert ref.shape == got.shape and err < IMG_TOL[mode]
    assert not got[geom.dom.cpu().numpy().reshape(got.shape) == 0].any()


def _tree(eng, flat):
    from bhnerf_amd import network
    tree = network.ParamTree(eng.unflatten(flat))
    tree.flat = flat
    return tree


def test_sum_of_an_image_term_and_the_prior(dev):
    """TrainStep.image + TrainStep.volume_prior: the call returns the image term's images unchanged, and the parameters after it
    are bitwise those of the two steps taken one after the other."""
    from bhnerf_amd import optimization
    pred, flat0, res = _predictor('bf16', dev)
    rt = _ray_set()
    rng = np.random.default_rng(2)
    t_frames = np.array([0.1, 0.4, 0.7])
    target = rng.uniform(0, 1e-3, (3, 8, 8)).astype(np.float32)
    image = lambda: optimization.TrainStep.image(t_frames, target, dtype='full')
    prior = lambda: optimization.TrainStep.volume_prior(16.0, resolution=res, weights={'tv': 1.0, 'l1': 0.1}, eps=1e-4, scale=3.0)
    idx = np.array([2, 0])
    both = image() + prior()
    a = _state(pred, flat0, rt)
    loss, a, imgs = both(a, rt, idx)
    b = _state(pred, flat0, rt)
    l1, b, imgs1 = image()(b, rt, idx)
    after_image = b.flat.clone()
    l2, b, zero = prior()(b, rt, idx)
    assert a.step == 2 and b.step == 2 and float((b.flat - after_image).abs().max()) > 0
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert imgs.shape == imgs1.shape == (1, 2, 8, 8) and torch.equal(imgs, imgs1) and zero.ndim == 0
    assert float(loss.sum()) == float((l1 + l2).sum())
    # test mode: the prior's loss is added once per call
    tl, _, timgs = both(a, rt, idx, update_state=False)
    t1 = image()(a, rt, idx, update_state=False)[0]
    t2 = prior()(a, rt, idx, update_state=False)[0]
    assert a.step == 2 and float(tl.sum()) == float((t1 + t2).sum()) and timgs.shape == imgs.shape
