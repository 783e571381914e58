"""BASELINE configs 3 and 5 at full size -- the polarised (Stokes I, Q, U) light-curve recoveries:

* config 3: 256 x 256 rays x 128 samples, 8 frames per step, 4x256 MLP, rmin = isco_pro(0.94), fov 40 M;
* config 5: 64 x 64 rays x 100 samples, 8 frames per step, 4x128 MLP, scale = rmax = 20, rmin = 6, z_width = 4
  (scripts/Fit_ALMA_LP_Apr11_SgrA_Flare.yaml).

Checked through size-independent properties: the f64 oracle on a random subset of rays (rays are independent), the
'lc' chi-square and its parameter gradient through the reference-shaped API on the full geometry against (i) the other
backward route (bhn_render_bwd, bitwise) and (ii) linearity in the light-curve residual.

Tolerances: f32 mode 1e-5 relative on images (north-star parity); bf16 mode 2e-2 of the per-Stokes image maximum."""
import numpy as np
import pytest
import torch

from gpu_support import chi2_step, dev, device_setup, problem_of  # noqa: F401
from mlp_problems import (STOKES_CONFIGS as CONFIGS, config_tree, flat_grad, oracle_images, oracle_inputs_of, ray_subset, rays_through_domain,
                          stokes_domain, stokes_problem, t64)
from oracle import oracle_np as onp
from oracle import oracle_torch as ot

pytestmark = pytest.mark.gpu
B = 8


def make_problem(name, dev):
    from bhnerf_amd import engine
    p = stokes_problem(name)
    return dict(p, tM0=engine.frame_offsets(p['t_frames'], 0.0, p['geo']['t_injection'], p['GM_c3'], dev))


def setup(p, mode, dev):
    c, geo = p['c'], p['geo']
    g = problem_of(p['tree'], geo, p['t_frames'], geo['t_injection'], stokes_domain(c), 3, 4, c['width'])
    pred, eng, geom, flat, _ = device_setup(g, mode, dev)
    eng.pack(flat)
    return pred, eng, geom


@pytest.mark.parametrize('name', ['config5', 'config3'])
def test_polarised_forward_against_oracle_on_a_ray_subset(dev, name):
    p = make_problem(name, dev)
    c = p['c']
    rays = np.random.default_rng(31).choice(c['H'] * c['W'], size=96, replace=False)
    ref = oracle_images(p, rays, stokes_domain(c), stokes=True)
    assert np.abs(ref).max() > 0
    # bf16: 1e-2 of the image maximum for Stokes I; Q and U are signed sums (cancellation along the ray), observed 1.05e-2
    for mode, tol in (('f32', 1e-5), ('bf16', 2e-2)):
        pred, eng, geom = setup(p, mode, dev)
        images = eng.render(geom, p['tM0'])                                              # (B, 3, R)
        assert images.shape == (B, 3, c['H'] * c['W'])
        got = images[:, :, torch.as_tensor(rays, device=dev)].cpu().numpy()
        for s in range(3):
            err = np.abs(got[:, s] - ref[:, s]).max() / np.abs(ref[:, s]).max()
            assert err <= tol, (mode, s, err)
        del images, eng, geom, pred
        torch.cuda.empty_cache()


@pytest.mark.parametrize('name', ['config5', 'config3'])
def test_polarised_lightcurve_gradient_properties(dev, name):
    """'lc' chi-square of all three Stokes light curves on the full geometry (bf16): reference-shaped training step,
    both backward routes bitwise equal, gradient linear in the residual."""
    from bhnerf_amd import network, optimization, units
    p = make_problem(name, dev)
    c, geo = p['c'], p['geo']
    pred, eng, geom = setup(p, 'bf16', dev)
    tM0 = p['tM0']
    images = eng.render(geom, tM0)
    lc = images.sum(dim=-1)                                                             # (B, 3)
    gen = torch.Generator(device=dev).manual_seed(4)
    r1 = (torch.rand((B, 3), device=dev, generator=gen) - 0.5) * lc.abs().max()
    r2 = (torch.rand((B, 3), device=dev, generator=gen) - 0.5) * lc.abs().max()
    bcast = lambda r: r[:, :, None].expand(B, 3, geom.R).contiguous()                    # d chi2 / d image of an 'lc' loss
    g1 = eng.render_bwd(geom, tM0, bcast(r1)).clone()
    assert torch.equal(eng.render_bwd(geom, tM0, bcast(r1)), g1)                       # reproducible, no float atomics
    g2 = eng.render_bwd(geom, tM0, bcast(r2)).clone()
    g12 = eng.render_bwd(geom, tM0, bcast(0.5 * r1 - 2.0 * r2)).clone()
    scale = float(torch.maximum(g1.abs().max(), g2.abs().max()))
    assert scale > 0 and float((g12 - (0.5 * g1 - 2.0 * g2)).abs().max()) <= 2e-2 * 2.5 * scale
    # the taped route (whole batch when the tape fits, frame groups otherwise) gives the bits of bhn_render_bwd
    group = B if eng.fits_tape(B, geom.P_eff) else eng.tape_group(B, geom.P_eff)
    acc = torch.zeros_like(g1)
    d = bcast(r1)
    for b0 in range(0, B, group):
        sl = slice(b0, min(b0 + group, B))
        eng.render_train(geom, tM0[sl])
        acc += eng.render_bwd_tape(geom, tM0[sl], d[sl].contiguous())
    assert float((acc - g1).abs().max()) <= 1e-4 * scale
    del images, acc, g12, g2, d
    torch.cuda.empty_cache()
    # the reference-shaped step on the same problem: loss equals the chi-square of the rendered light curves
    rt = network.raytracing_args(dict(x=geo['coords'][0], y=geo['coords'][1], z=geo['coords'][2], dtau=geo['dtau'], Sigma=geo['Sigma'],
                                      t=geo['t_geos'], g=geo['g']), geo['Omega'], geo['t_injection'], 0.0 * units.hr, J=geo['J'])
    target = (lc * 0.9).cpu().numpy()
    sigma = float(lc.abs().mean()) * 0.1
    step = optimization.TrainStep.image(p['t_frames'] * units.hr, target, sigma=sigma, dtype='lc')
    opt = optimization.Optimizer({'num_iters': 2, 'lr_init': 1e-4, 'lr_final': 1e-4}, pred, rt)
    opt.state.flat.copy_(eng.flatten(p['tree']).to(opt.state.flat))
    loss, _, frames = step(opt.state, rt, np.arange(B), update_state=False)
    want = float((((lc - torch.as_tensor(target, device=dev)) / sigma) ** 2).sum())
    assert abs(float(torch.as_tensor(loss).sum()) - want) <= 2e-2 * want


def test_config3_render_with_reference_pinned_J(dev):
    """BASELINE config 3's polarised render with REAL Kerr factors instead of synthetic ones: spin-0.94 geodesics of the own
    tracer (60 deg, 40 M field of view, 64 x 64 rays x 128 samples), Doppler factor and Stokes factors J = (I, Q, U) from
    bhnerf_amd/kgeo.py -- the functions fixture g12 pins to the reference's own kgeo.py:199-519 -- through the fused HIP
    render against the float64 oracle on 96 rays, both arithmetic modes."""
    from bhnerf_amd import constants, engine, geodesics, kgeo, network
    spin, inc, fov, NA, NG = 0.94, np.deg2rad(60.0), 40.0, 64, 128
    geos = geodesics.image_plane_geos(spin, inc, (-fov / 2, fov / 2), (-fov / 2, fov / 2), ngeo=NG, num_alpha=NA, num_beta=NA)
    r = np.asarray(geos.r)
    Omega = 1.0 / (np.maximum(r, 2.1) ** 1.5 + spin)                                    # prograde Keplerian (utils-style), capped inside the ISCO
    with np.errstate(all='ignore'):
        umu = kgeo.azimuthal_velocity_vector(geos, Omega)
        g = kgeo.doppler_factor(geos, umu)
        b = kgeo.magnetic_field_fluid_frame(geos, umu, 0.0, 1.0, 0.0)
        domain = (np.abs(geos.z) < 4.0) & (r > 2.024) & (r < fov / 2)                    # unit mean field strength over the recovery
        b = b / np.sqrt((b[domain] ** 2).sum(axis=-1)).mean()                            # domain, as alma.py:52-54 normalises it
        J = np.nan_to_num(kgeo.parallel_transport(geos, umu, g, b, Q_frac=0.85, V_frac=0), 0.0)
    assert J.shape == (3, NA, NA, NG) and np.abs(J[1][domain]).max() > 0.1 and np.abs(J[2][domain]).max() > 0.1
    f32 = lambda v: np.ascontiguousarray(np.nan_to_num(np.asarray(v, dtype=np.float64)), dtype=np.float32)
    coords = np.stack([f32(geos.x), f32(geos.y), f32(geos.z)])
    arrs = dict(Omega=f32(Omega), t_geos=f32(geos.t), g=f32(g), dtau=f32(geos.dtau), Sigma=f32(geos.Sigma), J=f32(J))
    t_frames = np.linspace(0.0, 1.7, 128)[:B]
    t_inj = -float(geos.r_o + fov / 4)
    GM = constants.GM_c3('hr')
    rng = np.random.default_rng(33)
    tree = config_tree(rng, 256)
    rmin, rmax, zw = 2.024, fov / 2, 4.0
    rays = np.random.default_rng(34).choice(NA * NA, size=96, replace=False)
    sub = lambda v: v.reshape((-1, NG))[rays].reshape(12, 8, NG).astype(np.float64)
    tree64 = {'MLP_0': {k: {kk: np.asarray(vv, dtype=np.float64) for kk, vv in v.items()} for k, v in tree['MLP_0'].items()}}
    e = onp.predictor_apply(tree64, t_frames, np.stack([sub(coords[i]) for i in range(3)]), sub(arrs['Omega']), 0.0, sub(arrs['t_geos']), t_inj,
                            GM_c3=GM, scale=rmax, rmin=rmin, rmax=rmax, z_width=zw)
    ref = onp.image_plane_prediction(e, np.stack([sub(arrs['J'][s]) for s in range(3)]), sub(arrs['g']), sub(arrs['dtau']),
                                     sub(arrs['Sigma'])).reshape(B, 3, 96)
    assert np.abs(ref[:, 0]).max() > 0 and np.abs(ref[:, 1]).max() > 0
    tM0 = engine.frame_offsets(t_frames, 0.0, t_inj, GM, dev)
    for mode, tol in (('f32', 1e-5), ('bf16', 2e-2)):
        pred = network.NeRF_Predictor(rmax, rmin, rmax, zw, net_depth=4, net_width=256, mode=mode, device=dev)
        eng = pred.engine()
        geom = pred.geometry(coords, arrs['Omega'], arrs['t_geos'], arrs['J'], arrs['g'], arrs['dtau'], arrs['Sigma'])
        eng.pack(eng.flatten(tree))
        got = eng.render(geom, tM0)[:, :, torch.as_tensor(rays, device=dev)].cpu().numpy()
        for s in range(3):
            err = np.abs(got[:, s] - ref[:, s]).max() / np.abs(ref[:, s]).max()
            assert err <= tol, (mode, s, err)


@pytest.mark.parametrize('name', ['config5', 'config3'])
def test_polarised_lightcurve_gradient_against_oracle_on_a_ray_subset(dev, name, capsys):
    """the gradient of the 'lc' chi-square of the three Stokes light curves at the shapes of configs 3 and 5
    (S = 3, point-compacted recovery domain, 8 frames) against torch.autograd on the float64 oracle, the loss restricted to
    256 rays of the full geometry (rays are independent; the light curve of a subset is the subset's own sum).  Config 5 is
    the reference-default 4x128 network: in bf16 its gradient comes out of bwd128_kernel (fused delta chain + dW), held
    here to the ORACLE and not to the library's other backward route.  Tolerances: f32 2e-5, bf16 3e-2 relative L2
    (observed values are printed).

    Why the f32 bound is 2e-5 and not north_star's 1e-5 (round 6): round 5 blamed the float rounding of the
    light curve's PIXEL SUM for the 1.3e-5 / 1.7e-5 observed here.  The sum (and the residual) are formed in double since round 6
    (chi2_image_kernel, 'lc' branch) -- and the figures did not move (config 5: 1.681e-5 before and after).  What limits them is
    upstream of the sum: the pixels themselves are float32 (each within 1e-6 of the image maximum of the oracle's), the Q and U
    light curves are sums of signed pixels that cancel to a few per cent of the I light curve, and chi^2's gradient is proportional
    to the residual of every light curve: a 2e-7 error of the pixels is a 1e-5 error of lc_Q.  The test prints that figure
    (`lc rel diff`); the float32 reference has the same pixels."""
    from bhnerf_amd import network
    p = make_problem(name, dev)
    c, geo = p['c'], p['geo']
    # 256 rays drawn among those that cross the recovery domain (most rays of the 40 M field of view miss |z| <= 4, r <= 20)
    g = ray_subset(geo, rays_through_domain(geo, c, 41), stokes=True)
    tr = ot.CpuTrainer(*oracle_inputs_of(p['tree'], g, geo['t_injection'], stokes_domain(c), 3, 4, GM_c3=p['GM_c3']))
    with torch.no_grad():
        lc0 = tr.forward(t64(p['t_frames'])).sum(dim=(-1, -2)).numpy()                    # (B, 3) light curves of the subset
    assert np.abs(lc0[:, 0]).max() > 0
    rng = np.random.default_rng(42)
    # A well-conditioned chi-square: residuals of at least 40 % of the light curve and ONE noise level (a fraction of the Stokes I
    # light curve) for all three Stokes parameters, as an instrument has.  (The Q and U light curves are sums of signed pixels
    # that cancel to a few per cent of I at these inclinations; with sigma_Q ~ |lc_Q| and a residual that is a small difference
    # of large numbers, the float32 rounding of the SUM over pixels is amplified by lc_I / lc_Q / residual fraction: a first
    # version of this test measured 8e-4 (config 5) and 6e-5 (config 3) in the f32 mode that way -- the arithmetic of an f32
    # light curve, which the f32 reference shares, not of the kernels.)
    target = lc0 * rng.uniform(0.3, 0.6, lc0.shape)
    sigma = np.abs(lc0[:, :1]).mean() * rng.uniform(0.05, 0.2, lc0.shape)
    offset = np.zeros_like(lc0)
    loss_ref, _, grads_ref = tr.loss_and_grad(t64(p['t_frames']), t64(target), t64(sigma), t64(offset), 1.0, 'lc')
    gref = flat_grad(grads_ref)
    assert np.linalg.norm(gref) > 0
    for mode, l2tol in (('f32', 2e-5), ('bf16', 3e-2)):
        pred = network.NeRF_Predictor(c['rmax'], c['rmin'], c['rmax'], c['z_width'], net_depth=4, net_width=c['width'], mode=mode, device=dev)
        gm = pred.geometry(g['coords'], g['Omega'], g['t_geos'], g['J'], g['g'], g['dtau'], g['Sigma'])
        assert gm.compact is not None and gm.S == 3                                       # the point-compacted layout, three Stokes planes
        rt = dict(g, t_start_obs=0.0, t_injection=float(geo['t_injection']))
        loss, images, gdev = chi2_step(pred, pred.engine().flatten(p['tree']), rt, p['t_frames'], target, sigma, offset, dt='lc')
        lc_dev = images.double().sum(dim=(-1, -2)).cpu().numpy()                            # the device's float32 pixels, summed in double
        lc_diff = np.abs(lc_dev - lc0).max(axis=0) / np.abs(lc0).max(axis=0)               # per Stokes parameter
        gdev = gdev.astype(np.float64)
        lerr = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
        err = float(np.linalg.norm(gdev - gref) / np.linalg.norm(gref))
        emax = float(np.abs(gdev - gref).max() / np.abs(gref).max())
        with capsys.disabled():
            print('\n[%s %s] lc gradient vs f64 oracle on 256 rays: rel L2 %.3e, max-norm %.3e, loss rel err %.3e (active fraction %.3f); lc rel diff I %.1e Q %.1e U %.1e'
                  % (name, mode, err, emax, lerr, gm.active_fraction, lc_diff[0], lc_diff[1], lc_diff[2]))
        assert lerr <= (1e-5 if mode == 'f32' else 3e-2)
        assert err < l2tol, (mode, err)


@pytest.mark.parametrize('name', ['config5', 'config5_128sq'])
def test_polarised_gradient_on_the_full_geometry_against_oracle(dev, name, capsys):
    """the oracle gradient on the FULL geometry, not on a 16 x 16-ray extract of it.  A 'full' chi-square whose
    noise level is infinite on every pixel but 256 (those pixels then contribute exactly 0 to the loss and to d loss / d image) is,
    for the oracle, a loss on 256 independent rays -- while the HIP path renders, records and back-propagates the WHOLE
    point-compacted ray set: every workgroup tile, the per-wave direct ray sums (`ray_span` <= 2) and the fused 4x128 backward
    run at their real sizes.  `config5` is BASELINE config 5 (64 x 64 rays x 100 samples: 8-group tiles); `config5_128sq` the same
    geometry on 128 x 128 rays -- more than 3,072 in-domain groups per frame, so the forward pair runs on 12-wave workgroups
    (PolBF16X) in front of bwd128_kernel.  Tolerances: f32 2e-5, bf16 3e-2 relative L2 (observed values are printed)."""
    from bhnerf_amd import network, synthetic
    c = dict(CONFIGS['config5'])
    if name == 'config5_128sq':
        c.update(H=128, W=128)
    geo = synthetic.synthetic_geodesics(c['H'], c['W'], c['G'], fov_M=c['fov'], inc_deg=c['inc'], spin=c['spin'], S=3, seed=3)
    p = make_problem('config5', dev)                                                    # (weights and frames of the 'config5' problem)
    HW = c['H'] * c['W']
    rays = rays_through_domain(geo, c, 43)
    tr = ot.CpuTrainer(*oracle_inputs_of(p['tree'], ray_subset(geo, rays, stokes=True), geo['t_injection'], stokes_domain(c), 3, 4, GM_c3=p['GM_c3']))
    with torch.no_grad():
        img0 = tr.forward(t64(p['t_frames'])).numpy()                                     # (B, 3, 16, 16)
    rng = np.random.default_rng(44)
    tgt_s = img0 * rng.uniform(0.3, 0.6, img0.shape)
    sig_s = np.abs(img0[:, :1]).mean() * rng.uniform(0.05, 0.2, img0.shape)
    loss_ref, _, grads_ref = tr.loss_and_grad(t64(p['t_frames']), t64(tgt_s), t64(sig_s), t64(np.zeros_like(img0)), 1.0, 'full')
    gref = flat_grad(grads_ref)
    assert np.linalg.norm(gref) > 0
    # the same loss on the full image plane: target 0 and sigma = inf wherever the oracle has no ray
    target = np.zeros((B, 3, HW), dtype=np.float32); sigma = np.full((B, 3, HW), np.inf, dtype=np.float32)
    target[:, :, rays] = tgt_s.reshape(B, 3, 256); sigma[:, :, rays] = sig_s.reshape(B, 3, 256)
    shp = (B, 3, c['H'], c['W'])
    for mode, l2tol in (('f32', 2e-5), ('bf16', 3e-2)):
        pred = network.NeRF_Predictor(c['rmax'], c['rmin'], c['rmax'], c['z_width'], net_depth=4, net_width=c['width'], mode=mode, device=dev)
        gm = pred.geometry(geo['coords'], geo['Omega'], geo['t_geos'], geo['J'], geo['g'], geo['dtau'], geo['Sigma'])
        assert gm.compact is not None and gm.S == 3 and gm.compact['ray_span'] in (1, 2)
        groups = (gm.P_eff + 31) // 32
        assert (groups >= 3072) == (name == 'config5_128sq')                              # the 12-wave tiles of the fused 4x128 forward pair
        loss, _, gdev = chi2_step(pred, pred.engine().flatten(p['tree']), dict(geo, t_start_obs=0.0), p['t_frames'], target.reshape(shp),
                                  sigma.reshape(shp), np.zeros(shp, dtype=np.float32))
        gdev = gdev.astype(np.float64)
        assert np.isfinite(gdev).all()
        lerr = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
        err = float(np.linalg.norm(gdev - gref) / np.linalg.norm(gref))
        with capsys.disabled():
            print('\n[%s %s, full geometry: %d in-domain groups per frame, ray span %d] gradient vs f64 oracle (loss on 256 rays): rel L2 %.3e, loss rel err %.3e'
                  % (name, mode, groups, gm.compact['ray_span'], err, lerr))
        assert lerr <= (1e-5 if mode == 'f32' else 3e-2)
        assert err < l2tol, (mode, err)
        del pred, gm, loss
        torch.cuda.empty_cache()
