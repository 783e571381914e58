"""The cases of the joint training step (optimization.TrainStep.joint, libbhnerf_jnt.so, include/bhnerf_jnt.h), shared by
tests/test_joint_cpu.py and tests/test_gpu_joint.py: the inputs of the fan-in kernel with NumPy's float32 left-to-right sum as their
reference, and the small training problem of the step tests.  Imported by the tests the way vol_reg_cases.py is; no test here.

Every comparison that stands on this file is bitwise: a float32 left-to-right sum has one correct answer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eht_uv_cases as E                                               # noqa: E402

MAX_TERMS = 8
SUM_N = (0, 1, 3, 4, 5, 1023, 1024, 1025)
SUM_K_CPU = (1, 2, 3, 8)
SUM_K_GPU = (1, 3, 8)


def sum_inputs(K, n, seed=0):
    """K float32 vectors of n elements: magnitudes over six decades, and by position +-0, subnormals, +inf and -inf (never both
    in one element: no NaN arises, so that bytes can be compared), values that cancel exactly, and triples whose sum depends on
    the order of the additions."""
    rng = np.random.default_rng([seed, K, n])
    a = (rng.normal(size=(K, n)) * 10.0 ** rng.uniform(-3, 3, size=(K, n))).astype(np.float32)
    i = np.arange(n)
    kind = i % 11
    for k in range(K):
        a[k, kind == 0] = 0.0 if k % 2 else -0.0
        a[k, kind == 1] = np.float32(1e-40) * np.float32(k + 1) * np.float32(-1.0 if k % 3 == 2 else 1.0)        # subnormal
    sel = np.where(kind == 2)[0]
    a[(sel // 11) % K, sel] = np.inf                                 # (index pairs: row (i // 11) % K of element i)
    sel = np.where(kind == 3)[0]
    a[(sel // 11) % K, sel] = -np.inf
    if K >= 2:
        sel = kind == 4
        a[K - 1, sel] = -a[0, sel]                                   # cancels against the first term (exactly when K == 2)
    if K >= 3:
        a[0, kind == 5], a[1, kind == 5], a[2, kind == 5] = 1e8, -1e8, 1.0        # ((a + b) + c) = 1, (a + (b + c)) = 0
        a[0, kind == 6], a[1, kind == 6], a[2, kind == 6] = 1.0, 1e8, -1e8        # ((a + b) + c) = 0, (a + (b + c)) = 1
        a[3:, (kind == 5) | (kind == 6)] = 0.0
    return a


def numpy_sum(srcs):
    """((srcs[0] + srcs[1]) + ...) in float32: THE reference."""
    acc = np.array(srcs[0], dtype=np.float32, copy=True)
    with np.errstate(all='ignore'):
        for s in srcs[1:]:
            acc = acc + np.asarray(s, dtype=np.float32)
    assert acc.dtype == np.float32
    return acc


def loss_inputs(K, seed=0):
    """K float32 losses whose sum depends on the order when K >= 3."""
    v = np.random.default_rng([seed, K]).uniform(0.1, 10.0, K).astype(np.float32)
    if K >= 3:
        v[:3] = (1e8, -1e8, 1.0)                             # ((a + b) + c) = 1, (a + (b + c)) = 0
    return v


def numpy_losses(v):
    """[left-to-right float32 sum | the K losses]."""
    total = np.float32(v[0])
    for x in v[1:]:
        total = np.float32(total + np.float32(x))
    return np.concatenate([[total], v]).astype(np.float32)


# ---- the small training problem of the step tests ----------------------------------------------------------------------------
H = W = 8
SAMPLES = 16
NT, BATCH = 4, 2
RES = 8
FOV_M = 16.0
HP = {'num_iters': 10, 'lr_init': 1e-3, 'lr_final': 1e-5, 'seed': 3}


def ray_set(stokes=False):
    from bhnerf_amd import network, synthetic, units
    geo = synthetic.synthetic_geodesics(H, W, SAMPLES, fov_M=FOV_M, seed=3, **(dict(S=3) if stokes else {}))
    return network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                        t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr,
                                   **(dict(J=geo['J']) if stokes else {}))


def predictor(mode, dev):
    """(a 4x128 NeRF with posenc_deg 3, its initial flat parameters); the domain 2 <= r <= 8, |z| <= 4 cuts the lattice of fov 16."""
    import torch
    from bhnerf_amd import network
    pred = network.NeRF_Predictor(8.0, 2.0, 8.0, 4.0, posenc_deg=3, net_depth=4, net_width=128, mode=mode, device=dev)
    params = pred.init_params(seed=3)
    with torch.no_grad():                                  # emission sigmoid(out - 10): a large bias makes the images visible
        pred.engine().unflatten(params.flat)['MLP_0']['Dense_4']['bias'] += 8.0
    return pred, params.flat.clone()


def new_state(pred, flat, rt):
    import torch
    from bhnerf_amd import optimization
    opt = optimization.Optimizer(HP, pred, rt)
    with torch.no_grad():
        opt.state.flat.copy_(flat)
    return opt.state


def t_frames():
    from bhnerf_amd import units
    return np.linspace(0.0, 0.5, NT) * units.hr


def uv_table(seed=21, stations=4):
    """((NT, 6, 2) float64 baselines in wavelengths, pairs (6, 2)): 6 baselines of 4 stations."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(NT, stations, 2)) * 0.5e9
    pairs = np.array([(i, j) for i in range(stations) for j in range(i + 1, stations)])
    return np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]]), pairs


def data_terms(image_scale=1.0, vis_scale=0.5, prior_scale=2.0):
    """The three terms of the hand-built step test -- image('full'), eht_uv('vis'), volume_prior({'tv': 1}) -- as TrainSteps."""
    from bhnerf_amd.optimization import TrainStep
    rng = np.random.default_rng(11)
    target = rng.uniform(0.0, 2e-3, (NT, H, W)).astype(np.float32)
    uv, _ = uv_table()
    vis = (1e-2 * (rng.normal(size=(NT, 6)) + 1j * rng.normal(size=(NT, 6)))).astype(np.complex64)
    image = TrainStep.image(t_frames(), target, sigma=1e-3, scale=image_scale, dtype='full')
    vis_step = TrainStep.eht_uv(t_frames(), vis, np.full((NT, 6), 5e-3, dtype=np.float32), uv, E.FOV, H, dtype='vis', scale=vis_scale)
    prior = TrainStep.volume_prior(FOV_M, resolution=RES, weights={'tv': 1.0}, eps=1e-4, scale=prior_scale)
    return image, vis_step, prior


def stokes_terms():
    """eht_closure('cphase+logcamp') on the I plane's data and eht_pol('m'): the combination of the --gains example."""
    from bhnerf_amd.optimization import TrainStep
    rng = np.random.default_rng(12)
    uv, pairs = uv_table()
    ntri, nquad = 4, 2                                      # every triangle of 4 stations, the 2 independent quadrangles
    data = {'cphase': (rng.uniform(-1.0, 1.0, (NT, 3, ntri)).astype(np.float32), np.full((NT, 3, ntri), 0.3, dtype=np.float32)),
            'logcamp': (rng.normal(0.0, 0.3, (NT, 3, nquad)).astype(np.float32), np.full((NT, 3, nquad), 0.2, dtype=np.float32))}
    for term in data:
        data[term][1][:, 1:] = np.inf                       # the Q and U planes of the closure step carry no weight
    closure = TrainStep.eht_closure(t_frames(), uv, E.FOV, H, pairs, data, scale=1.5)
    m = (0.3 * (rng.normal(size=(NT, 6)) + 1j * rng.normal(size=(NT, 6)))).astype(np.complex64)
    pol = TrainStep.eht_pol(t_frames(), uv, E.FOV, H, {'m': (m, np.full((NT, 6), 0.1, dtype=np.float32))}, scale=0.7)
    return closure, pol
