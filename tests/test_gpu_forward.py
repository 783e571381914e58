"""GPU parity tests (through the C ABI) of the forward half of the hot path against the oracle and
the golden vectors produced by the reference's own code.

Tolerances: f32 mode 1e-5 relative to the largest output (north-star tolerance); bf16 mode 3e-2
(bf16 operands, f32 accumulate: the emission's relative error equals the absolute error of the
pre-activation, DESIGN.md "numerics")."""
import numpy as np
import pytest
import torch

from conftest import golden_tree
from gpu_support import predictor_of
from mlp_bounds import IMG_TOL, TOL, relerr
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
PRED = ['a', 'b', 'c', 'd', 'e', 'f']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda:0')


def test_selftest_lane_maps(dev):
    from bhnerf_amd import _hip
    res, msg = _hip.selftest()
    assert res[:5] == [0, 0, 0, 0, 0] and res[7] == 0, (res, msg)


@pytest.mark.parametrize('N,R,G', [(1, 7, 5), (6, 33, 64), (3, 50, 100), (2, 19, 128), (2, 5, 300), (1, 3, 1024), (4, 9, 66)])
def test_radiative_transfer_standalone(dev, N, R, G):
    from bhnerf_amd import kgeo
    rng = np.random.default_rng(N * 1000 + R * 10 + G)
    e = rng.uniform(0, 1, (N, R, 1, G)).astype(np.float32)
    g, dtau, Sigma = (rng.uniform(0.5, 1.5, (R, 1, G)).astype(np.float32) for _ in range(3))
    ref = onp.radiative_trasfer(e.astype(np.float64), g.astype(np.float64), dtau.astype(np.float64), Sigma.astype(np.float64))
    et = torch.tensor(e, device=dev, requires_grad=True)
    out = kgeo.radiative_trasfer(et, torch.tensor(g, device=dev), torch.tensor(dtau, device=dev), torch.tensor(Sigma, device=dev))
    assert out.shape == ref.shape
    assert relerr(out.detach().cpu().numpy(), ref) < 2e-6
    up = rng.normal(size=ref.shape).astype(np.float32)
    out.backward(torch.tensor(up, device=dev))
    de_ref = up[..., None].astype(np.float64) * (g.astype(np.float64) ** 2 * dtau * Sigma)
    assert relerr(et.grad.cpu().numpy(), de_ref) < 2e-6
    # scalars for g/dtau/Sigma (notebooks pass dtau=1.0) and numpy inputs follow the reference host path
    out2 = kgeo.radiative_trasfer(torch.tensor(e, device=dev), 1.3, 1.0, 0.5)
    assert relerr(out2.cpu().numpy(), onp.radiative_trasfer(e.astype(np.float64), 1.3, 1.0, 0.5)) < 2e-6
    assert np.allclose(kgeo.radiative_trasfer(e, g, dtau, Sigma), ref, rtol=1e-5)


def test_radiative_transfer_golden(dev, golden):
    from bhnerf_amd import kgeo
    g = golden('g4_rt')
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    out = kgeo.radiative_trasfer(t(g['emission']), t(g['g']), t(g['dtau']), t(g['Sigma']))
    assert relerr(out.cpu().numpy(), g['out_arrays']) < 2e-6


def test_geom_prepare(dev, golden):
    from bhnerf_amd import engine
    g = golden('g5_predict_b')
    hp = g['hparams']
    geo = engine.RayGeometry(g['coords'], g['Omega'], g['g'], g['dtau'], g['Sigma'], g['t_geos'], g['J'], hp[1], hp[2], hp[3], dev)
    w_ref = (g['g'] ** 2 * g['dtau'] * g['Sigma'])[None] * g['J']
    assert relerr(geo.w.cpu().numpy().reshape(w_ref.shape), w_ref) < 1e-6
    c = g['coords'].astype(np.float32)
    r2 = (c ** 2).sum(0)
    dom = ~((r2 < np.float32(hp[1]) ** 2) | (r2 > np.float32(hp[2]) ** 2) | (np.abs(c[2]) > hp[3]))
    # the mask equals the float64 reference's except where the decision lies within f32 rounding (none in this fixture)
    from conftest import mask_tie_points
    ties = mask_tie_points(g)[0]
    dom64 = ~((g['coords'] ** 2).sum(0) < hp[1] ** 2) & ~((g['coords'] ** 2).sum(0) > hp[2] ** 2) & ~(np.abs(g['coords'][2]) > hp[3])
    bad = (geo.dom.cpu().numpy().reshape(dom.shape) != dom64) & ~ties
    assert not bad.any(), int(bad.sum())
    assert (geo.dom.cpu().numpy().reshape(dom.shape) != dom).sum() <= ties.sum()
    assert 0.0 < geo.active_fraction < 1.0


def _predictor(g, mode, dev):
    return predictor_of(g, mode, dev), golden_tree(g)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('tag', PRED)
def test_predictor_apply_golden(dev, golden, tag, mode):
    """NeRF_Predictor.apply == the reference's NeRF_Predictor.__call__ output on identical weights."""
    from bhnerf_amd import units
    g = golden('g5_predict_' + tag)
    pred, tree = _predictor(g, mode, dev)
    e = pred.apply({'params': tree}, g['t_frames'], units.hr, g['coords'].astype(np.float32), g['Omega'].astype(np.float32),
                   float(g['t_start_obs']), g['t_geos'].astype(np.float32), float(g['t_injection']))
    assert tuple(e.shape) == g['emission'].shape
    e = e.cpu().numpy()
    # the masks (domain, injection) agree exactly except where the reference's decision lies within f32 rounding
    from conftest import mask_tie_points
    ties = mask_tie_points(g).reshape(e.shape)
    mismatch = (e == 0) != (g['emission'] == 0)
    assert not (mismatch & ~ties).any(), int((mismatch & ~ties).sum())
    same = ~mismatch
    assert relerr(e[same], g['emission'][same]) < TOL[mode], relerr(e[same], g['emission'][same])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('tag', PRED)
def test_image_plane_prediction_golden(dev, golden, tag, mode):
    from bhnerf_amd import network, units
    g = golden('g5_predict_' + tag)
    pred, tree = _predictor(g, mode, dev)
    f = lambda k: g[k].astype(np.float32)
    J = f('J') if g['J'].ndim else 1.0
    with torch.no_grad():
        images = network.image_plane_prediction(tree, pred.apply, g['t_frames'], f('coords'), f('Omega'), J, f('g'),
                                                f('dtau'), f('Sigma'), float(g['t_start_obs']), f('t_geos'),
                                                float(g['t_injection']), units.hr)
    assert tuple(images.shape) == g['images'].shape          # incl. the b=1 squeeze quirk (tag d)
    # a boundary tie may flip one sample of a ray: pixels whose ray holds no tie point are held to the tolerance
    from conftest import mask_tie_points
    tie_ray = mask_tie_points(g).any(axis=-1)                                  # (b, H, W)
    got, ref = images.cpu().numpy(), g['images']
    S = g['J'].shape[0] if g['J'].ndim else 0
    clean = ~np.broadcast_to(tie_ray[:, None] if S else tie_ray, (len(g['t_frames']),) + ((S,) if S else ()) + tie_ray.shape[1:]).reshape(ref.shape)
    assert clean.any()
    assert np.abs(got - ref)[clean].max() / np.abs(ref).max() < IMG_TOL[mode]


def test_chi2_and_adam(dev):
    from bhnerf_amd import engine
    rng = np.random.default_rng(5)
    B, S, R = 3, 2, 77
    img, tgt, off = (rng.normal(size=(B, S, R)).astype(np.float32) for _ in range(3))
    sig = rng.uniform(0.5, 2, (B, S, R)).astype(np.float32)
    t = lambda x: torch.tensor(x, device=dev)
    loss, dimg = engine.chi2_image(t(img), t(tgt), t(sig), t(off), 0.7, 'full')
    ref = onp.loss_image(img.astype(np.float64), tgt, sig, off, 0.7, 'full')
    assert abs(loss.item() - ref) < 1e-5 * ref
    assert relerr(dimg.cpu().numpy(), 2 * 0.7 * (img - tgt - off) / sig ** 2) < 1e-5
    loss, dimg = engine.chi2_image(t(img), t(tgt[..., 0]), t(sig[..., 0]), t(off[..., 0]), 0.7, 'lc')
    ref = onp.loss_image(img.astype(np.float64)[..., None], tgt[..., 0], sig[..., 0], off[..., 0], 0.7, 'lc')
    assert abs(loss.item() - ref) < 1e-4 * ref
    d = (img.astype(np.float64).sum(-1) - tgt[..., 0] - off[..., 0]) / sig[..., 0] ** 2
    assert relerr(dimg.cpu().numpy(), np.broadcast_to((2 * 0.7 * d)[..., None], img.shape)) < 1e-4
    with pytest.raises(AttributeError):
        engine.chi2_image(t(img), t(tgt), t(sig), t(off), 1.0, 'nope')
    # Adam: three steps with linear decay == the oracle's optax restatement
    p0 = rng.normal(size=1000); p = p0.copy(); m = np.zeros_like(p); v = np.zeros_like(p)
    tp, tm, tv = t(p0.astype(np.float32)), torch.zeros(1000, device=dev), torch.zeros(1000, device=dev)
    for step in range(1, 4):
        gnp = rng.normal(size=1000)
        lr = onp.linear_lr(step - 1, 1e-2, 1e-4, 3)
        p, m, v = onp.adam_step(p, gnp * 0.5, m, v, step, lr)
        engine.adam_step(tp, t(gnp.astype(np.float32)), tm, tv, step, lr, grad_scale=0.5)
    assert relerr(tp.cpu().numpy(), p) < 1e-5


def test_fail_loud_on_cpu_tensors():
    from bhnerf_amd import _hip, kgeo
    with pytest.raises(_hip.HipError):
        kgeo.radiative_trasfer(torch.zeros(2, 3, 4), 1.0, 1.0, 1.0)


def test_domain_compaction_skips_groups_but_not_results(dev):
    """A thin-slab domain (as in the ALMA fits: rmin=6, rmax=20, z_width=4) leaves most 32-point groups
    empty; the compacted kernels must still reproduce the oracle on every pixel and every emission."""
    from bhnerf_amd import network, synthetic, units
    from oracle import oracle_np as onp2
    H, W, G, B = 12, 10, 64, 2
    geo = synthetic.synthetic_geodesics(H, W, G, fov_M=40.0, inc_deg=12.0, seed=5)
    rng = np.random.default_rng(2)
    tree = onp2.he_uniform_params(rng, 4, 64, 21)
    t_frames = np.array([0.2, 0.9])
    pred = network.NeRF_Predictor(20.0, 6.0, 20.0, 4.0, net_width=64, mode='f32', device=dev)
    rt = (geo['coords'], geo['Omega'], 1.0, geo['g'], geo['dtau'], geo['Sigma'], 0.0, geo['t_geos'], geo['t_injection'])
    geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], None, geo['g'], geo['dtau'], geo['Sigma'])
    assert geom.groups is not None and geom.visited_fraction < 0.6 and geom.active_fraction < geom.visited_fraction
    f64 = {k: np.asarray(v, dtype=np.float64) for k, v in geo.items() if not np.isscalar(v)}
    tree64 = {'MLP_0': {k: {kk: vv.astype(np.float64) for kk, vv in v.items()} for k, v in tree['MLP_0'].items()}}
    e_ref = onp2.predictor_apply(tree64, t_frames, f64['coords'], f64['Omega'], 0.0, f64['t_geos'], geo['t_injection'],
                                 scale=20.0, rmin=6.0, rmax=20.0, z_width=4.0, net_depth=4)
    img_ref = onp2.image_plane_prediction(e_ref, 1.0, f64['g'], f64['dtau'], f64['Sigma'])
    e = pred.apply({'params': tree}, t_frames, units.hr, geo['coords'], geo['Omega'], 0.0, geo['t_geos'], geo['t_injection'])
    with torch.no_grad():
        img = network.image_plane_prediction(tree, pred.apply, t_frames, *rt, units.hr)
    e = e.cpu().numpy()
    assert ((e == 0) != (e_ref == 0)).mean() < 0.01
    same = (e == 0) == (e_ref == 0)
    assert relerr(e[same], e_ref[same]) < 1e-5 and relerr(img.cpu().numpy(), img_ref) < 2e-5


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_point_compaction_of_the_domain_mask_changes_nothing(dev, mode):
    """engine.RayGeometry.compact: the fused kernels evaluate only the in-domain samples (ray index per point instead of
    p / G).  Images, per-point emission and parameter gradients must equal the dense evaluation (out-of-domain samples
    have emission 0, emission.py:370-373): same per-point arithmetic, different tiling -> f32 summation-order noise only."""
    from bhnerf_amd import constants, engine, network, synthetic
    geo = synthetic.synthetic_geodesics(24, 20, 50, S=3, seed=4)          # ragged: 50 samples per ray
    rng = np.random.default_rng(2)
    tree = onp.he_uniform_params(rng, 4, 128, 21, dtype=np.float32)
    tree['MLP_0']['Dense_4']['bias'] = tree['MLP_0']['Dense_4']['bias'] + 9.0
    tM0 = engine.frame_offsets(np.linspace(0.0, 0.7, 3), 0.0, geo['t_injection'], constants.GM_c3('hr'), dev)
    out = {}
    for compact in (False, True):
        engine.COMPACT_POINTS = compact
        try:
            pred = network.NeRF_Predictor(8.0, 3.0, 7.0, 2.5, net_depth=4, net_width=128, mode=mode, device=dev)
            eng = pred.engine()
            geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], geo['J'], geo['g'], geo['dtau'], geo['Sigma'])
        finally:
            engine.COMPACT_POINTS = True
        assert (geom.compact is not None) == compact
        eng.pack(eng.flatten(tree))
        gen = torch.Generator(device=dev).manual_seed(1)
        d = torch.rand((3, 3, geom.R), device=dev, generator=gen) - 0.4
        out[compact] = (eng.render(geom, tM0).clone(), eng.predict(geom, tM0).clone(), eng.render_bwd(geom, tM0, d).clone(),
                        geom.visited_fraction, geom.active_fraction)
    (img0, e0, g0, vis0, act0), (img1, e1, g1, vis1, act1) = out[False], out[True]
    assert act0 == act1 and vis1 < vis0 and vis1 <= act1 + 32.0 / geom.P          # only the padding is extra
    assert float(img0.abs().max()) > 0
    assert torch.equal(e0, e1)                                                       # per-point values are bit-identical
    assert float((img0 - img1).abs().max()) <= 2e-6 * float(img0.abs().max())
    assert float((g0 - g1).abs().max()) <= (1e-5 if mode == 'f32' else 1e-4) * float(g0.abs().max())


@pytest.mark.parametrize('mode,G', [('bf16', 100), ('bf16', 128), ('bf16', 250), ('f32', 100), ('f32', 128)])
def test_render_is_bitwise_reproducible_for_long_and_masked_rays(dev, mode, G):
    """Images are sums over the ray in a fixed order (RaySum, fused_common.h): the segment sums of a workgroup tile are
    combined in wave order and a pixel receives at most two (commutative) atomic adds for rays of up to 257 samples in bf16
    mode / 129 in f32 mode -- also with a masked domain (point compaction) and with Stokes planes.  Round 1 issued one
    float atomic per 32-sample segment: 3+ adds per pixel at these sizes, order-dependent."""
    from bhnerf_amd import constants, engine, network, synthetic
    H = W = 48
    geo = synthetic.synthetic_geodesics(H, W, G, fov_M=16.0, inc_deg=60.0, seed=5)
    rng = np.random.default_rng(1)
    J = rng.uniform(0.5, 1.5, (3, H, W, G)).astype(np.float32)
    for dom in ((8.0, 2.0, 8.0, 4.0), (8.0, 0.0, np.inf, np.inf)):            # masked (compacted) and all-active
        pred = network.NeRF_Predictor(*dom, net_depth=4, net_width=64, mode=mode, device=dev)
        eng = pred.engine()
        flat = eng.flatten(network.MLP(4, 64).init(3, 21))
        with torch.no_grad():
            eng.unflatten(flat)['MLP_0']['Dense_4']['bias'] += 8.0
        eng.pack(flat)
        geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], J, geo['g'], geo['dtau'], geo['Sigma'])
        tM0 = engine.frame_offsets(np.linspace(0, 1, 3), 0.0, geo['t_injection'], constants.GM_c3('hr'), dev)
        ref = eng.render(geom, tM0).clone()
        assert float(ref.abs().max()) > 0
        for _ in range(3):
            assert torch.equal(eng.render(geom, tM0), ref)
        assert torch.equal(eng.render_train(geom, tM0), ref)                  # the training forward sums the same way


@pytest.mark.parametrize('mode,width', [('bf16', 128), ('bf16', 256), ('f32', 64)])
def test_compacted_rays_within_two_groups_skip_the_combine(dev, mode, width):
    """bhn_geom.ray_span (ABI 4): on a point-compacted polarised ray set whose rays lie within two 32-point groups each
    (BASELINE configs 3 and 5 do) every wave adds its ray segments straight to the pixels -- still bitwise reproducible (a
    pixel gets at most two partial sums), and the same image as the per-tile combine through LDS (ray_span 0: unknown)."""
    from bhnerf_amd import network, synthetic, engine as E, constants
    H = W = 48; G = 100
    geo = synthetic.synthetic_geodesics(H, W, G, fov_M=40.0, inc_deg=12.0, spin=0.0, S=3, seed=3)
    pred = network.NeRF_Predictor(20.0, 6.0, 20.0, 4.0, net_depth=4, net_width=width, mode=mode, device=dev)
    geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], geo['J'], geo['g'], geo['dtau'], geo['Sigma'])
    assert geom.compact is not None and geom.compact['ray_span'] in (1, 2) and geom.S == 3
    eng = pred.engine()
    eng.pack(eng.flatten(network.MLP(4, width).init(3, 21)))
    tM0 = E.frame_offsets(np.linspace(0.0, 1.5, 5), 0.0, geo['t_injection'], constants.GM_c3('hr'), dev)
    imgs = [eng.render(geom, tM0).clone() for _ in range(3)]
    train = eng.render_train(geom, tM0).clone()
    assert float(imgs[0].abs().max()) > 0 and all(torch.equal(imgs[0], v) for v in imgs[1:]) and torch.equal(imgs[0], train)
    span = geom.compact['ray_span']
    geom.compact['ray_span'] = 0
    try:
        ref = eng.render(geom, tM0).clone()
    finally:
        geom.compact['ray_span'] = span
    assert torch.allclose(imgs[0], ref, rtol=2e-6, atol=1e-7 * float(ref.abs().max()))


def test_two_threads_two_streams_are_independent(dev):
    """ABI conventions (include/bhnerf_hip.h): no global mutable state except the thread-local error string and
    per-device one-time caches, so two host threads may drive the library on two streams of one device at the same time.
    Each thread owns a predictor (packed weights, outputs) and a stream and renders repeatedly; every result must equal
    the single-threaded one bit for bit."""
    import threading
    from bhnerf_amd import constants, engine, network, synthetic
    H = W = 32; G = 64
    geo = synthetic.synthetic_geodesics(H, W, G, fov_M=16.0, inc_deg=60.0, seed=7)
    tM0 = engine.frame_offsets(np.linspace(0, 1, 4), 0.0, geo['t_injection'], constants.GM_c3('hr'), dev)

    def make(seed, width, mode):
        pred = network.NeRF_Predictor(8.0, 2.0, 8.0, 4.0, net_depth=4, net_width=width, mode=mode, device=dev)
        eng = pred.engine()
        flat = eng.flatten(network.MLP(4, width).init(seed, 21))
        with torch.no_grad():
            eng.unflatten(flat)['MLP_0']['Dense_4']['bias'] += 8.0
        geom = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], None, geo['g'], geo['dtau'], geo['Sigma'])
        return eng, flat, geom

    jobs = [make(1, 128, 'bf16'), make(2, 256, 'bf16')]              # two different kernels (template instantiations)
    refs = []
    for eng, flat, geom in jobs:
        eng.pack(flat)
        refs.append(eng.render(geom, tM0).clone())
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            eng, flat, geom = jobs[k]
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for _ in range(20):
                    eng.pack(flat)
                    out = eng.render(geom, tM0)
                    dimg = torch.ones_like(out)
                    g1 = eng.render_bwd(geom, tM0, dimg)
                    stream.synchronize()
                    if not torch.equal(out, refs[k]) or not torch.isfinite(g1).all():
                        errors.append((k, 'mismatch'))
        except Exception:                                              # noqa: BLE001
            import traceback
            errors.append((k, traceback.format_exc()))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
