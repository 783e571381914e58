"""BASELINE config 2 at full size (128x128 rays x 64 samples, 8 frames per step, 4x256 MLP) through properties that do
not need the whole oracle: the oracle on a random subset of rays (every ray is independent), agreement of the two
forward routes (fused render vs predictor + stand-alone ray sum), linearity and frame-additivity of the parameter
gradient, the two backward routes (recorded tape vs bhn_render_bwd), run-to-run bitwise reproducibility, and the
oracle's gradient on a problem restricted to the same subset of rays.

Every test runs on two recovery domains: the tutorial-style masked one (rmin 2, rmax 8, |z| <= 4: point-compacted layout,
ray sums combined per workgroup tile) and the ALL-ACTIVE one of bench.py's headline line (rmin 0, rmax = z_width = inf:
dense layout, every sample through the MLP, per-tile-atomic ray sums) -- the exact variant the benchmark times.

Tolerances: f32 mode 1e-5 relative on images (north-star parity mode); bf16 mode 2e-2 of the image maximum
(bf16 activations, measured 3e-3); gradients: bf16 5e-2 relative L2 against the f64 oracle on 256 rays."""
import numpy as np
import pytest
import torch

from gpu_support import chi2_step, dev, device_setup, problem_of  # noqa: F401
from mlp_problems import CONFIG2, CONFIG2_DOMAINS as DOMAINS, config_problem, flat_grad, oracle_images, oracle_inputs_of, ray_subset, t64
from oracle import oracle_torch as ot

pytestmark = pytest.mark.gpu
H, W, G, B = CONFIG2['H'], CONFIG2['W'], CONFIG2['G'], len(CONFIG2['t_frames'])


@pytest.fixture(scope='module')
def problem(dev):
    from bhnerf_amd import engine
    p = config_problem(**CONFIG2)
    return dict(p, tM0=engine.frame_offsets(p['t_frames'], 0.0, p['geo']['t_injection'], p['GM_c3'], dev))


@pytest.fixture(params=['masked', 'all_active'])
def domain(request):
    return request.param


def setup(problem, mode, dev, domain='masked'):
    g = problem_of(problem['tree'], problem['geo'], problem['t_frames'], problem['geo']['t_injection'], DOMAINS[domain], 3, 4, CONFIG2['width'])
    pred, eng, geom, flat, _ = device_setup(g, mode, dev)
    eng.pack(flat)
    if domain == 'all_active':
        assert geom.visited_fraction == 1.0 and geom.active_fraction > 0.99        # dense layout, (nearly) every sample live
    else:
        assert geom.visited_fraction < 0.9                                          # point-compacted layout
    return pred, eng, geom


@pytest.mark.parametrize('mode,tol', [('f32', 1e-5), ('bf16', 1e-2)])
def test_forward_full_size_against_oracle_on_a_ray_subset_and_both_routes(dev, problem, mode, tol, domain):
    from bhnerf_amd import kgeo
    pred, eng, geom = setup(problem, mode, dev, domain)
    images = eng.render(geom, problem['tM0'])[:, 0]                                   # (B, R)
    assert images.shape == (B, H * W) and float(images.max()) > 0
    rays = np.random.default_rng(11).choice(H * W, size=96, replace=False)
    ref = oracle_images(problem, rays, DOMAINS[domain])
    got = images[:, torch.as_tensor(rays, device=dev)].cpu().numpy()
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    # route 2: emission (B,P) from the predictor kernel, integrated by the stand-alone ray-sum kernel
    e = eng.predict(geom, problem['tM0']).reshape(B, H, W, G)
    geo = problem['geo']
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev)
    images2 = kgeo.radiative_trasfer(e, t(geo['g']), t(geo['dtau']), t(geo['Sigma'])).reshape(B, H * W)
    assert float((images2 - images).abs().max()) <= 2e-6 * float(images.abs().max())
    # the training forward renders the same images (and records the tape)
    images3 = eng.render_train(geom, problem['tM0'])[:, 0]
    assert float((images3 - images).abs().max()) <= 2e-6 * float(images.abs().max())


def test_backward_full_size_properties_bf16(dev, problem, domain):
    pred, eng, geom = setup(problem, 'bf16', dev, domain)
    tM0 = problem['tM0']
    gen = torch.Generator(device=dev).manual_seed(3)
    d1 = torch.rand((B, 1, geom.R), device=dev, generator=gen) - 0.5
    d2 = torch.rand((B, 1, geom.R), device=dev, generator=gen) - 0.5
    assert eng.fits_tape(B, geom.P_eff)
    eng.render_train(geom, tM0)
    g1 = eng.render_bwd_tape(geom, tM0, d1).clone()
    g1_again = eng.render_bwd_tape(geom, tM0, d1).clone()
    assert torch.equal(g1, g1_again)                                    # no float atomics: bitwise reproducible
    g2 = eng.render_bwd_tape(geom, tM0, d2).clone()
    g12 = eng.render_bwd_tape(geom, tM0, (0.5 * d1 - 2.0 * d2).contiguous()).clone()
    scale = float(torch.maximum(g1.abs().max(), g2.abs().max()))
    assert scale > 0
    # linear in the upstream gradient up to the bf16 rounding of the deltas on the tape
    assert float((g12 - (0.5 * g1 - 2.0 * g2)).abs().max()) <= 2e-2 * 2.5 * scale
    # the other backward route (bhn_render_bwd: forward again + chain, frame groups) gives the same bits
    g1_rec = eng.render_bwd(geom, tM0, d1).clone()
    assert torch.equal(g1_rec, g1)
    # frames are independent: the gradient of the batch is the sum over frame groups
    parts = torch.zeros_like(g1)
    for b0 in range(0, B, 3):
        sl = slice(b0, min(b0 + 3, B))
        eng.render_train(geom, tM0[sl])
        parts += eng.render_bwd_tape(geom, tM0[sl], d1[sl].contiguous())
    assert float((parts - g1).abs().max()) <= 1e-5 * scale + 1e-3 * float((parts - g1).abs().mean() + 1e-30) + 2e-6 * scale


def test_gradient_full_width_against_oracle_on_a_ray_subset(dev, problem, domain, capsys):
    """4x256 network, 256 rays of the full geometry x 64 samples x 8 frames: chi^2 gradient vs torch.autograd on the f64 oracle,
    in the parity mode (f32), the throughput mode (bf16) and the opt-in 8-bit-tape mode (bf16_t8: bf16 arithmetic, e4m3 dW
    operands) -- the observed errors are printed."""
    from bhnerf_amd import network
    geo = problem['geo']
    scale, rmin, rmax, z_width = DOMAINS[domain]
    rays = np.sort(np.random.default_rng(12).choice(H * W, size=256, replace=False))
    g = ray_subset(geo, rays)
    rng = np.random.default_rng(13)
    target = rng.uniform(0, 1e-2, (B, 16, 16)); sigma = rng.uniform(0.5, 2.0, (B, 16, 16)); offset = np.zeros((B, 16, 16))
    tr = ot.CpuTrainer(*oracle_inputs_of(problem['tree'], g, geo['t_injection'], DOMAINS[domain], 3, 4, GM_c3=problem['GM_c3']))
    loss_ref, _, grads_ref = tr.loss_and_grad(t64(problem['t_frames']), t64(target), t64(sigma), t64(offset), 1.0, 'full')
    gref = flat_grad(grads_ref)
    for mode, l2tol in (('f32', 2e-5), ('bf16', 2e-2), ('bf16_t8', 2.5e-2)):
        pred = network.NeRF_Predictor(scale, rmin, rmax, z_width, net_depth=4, net_width=256, mode=mode, device=dev)
        rt = dict(g, J=1.0, t_start_obs=0.0, t_injection=float(geo['t_injection']))
        loss, _, gdev = chi2_step(pred, pred.engine().flatten(problem['tree']), rt, problem['t_frames'], target, sigma, offset)
        gdev = gdev.astype(np.float64)
        assert abs(loss.item() - loss_ref.item()) <= (1e-5 if mode == 'f32' else 2e-2) * abs(loss_ref.item())
        err = float(np.linalg.norm(gdev - gref) / np.linalg.norm(gref))
        with capsys.disabled():
            print('\n[config 2, %s, %s] gradient vs f64 oracle on 256 rays: rel L2 %.3e, max-norm %.3e' % (domain, mode, err, float(np.abs(gdev - gref).max() / np.abs(gref).max())))
        assert err < l2tol, (mode, err)


def test_taped_step_is_bitwise_stable_under_hbm_contention(dev, problem, domain):
    """The weight / tape rings use counted s_waitcnt vmcnt (in-order completion of the LDS-DMA loads and the tape stores,
    DESIGN.md 4.2-4.3).  A wait that is one operation too lax shows up as run-to-run differences once the memory system
    is perturbed: every second repetition runs against a copy stream that saturates HBM."""
    pred, eng, geom = setup(problem, 'bf16', dev, domain)
    tM0 = problem['tM0']
    gen = torch.Generator(device=dev).manual_seed(9)
    d = torch.rand((B, 1, geom.R), device=dev, generator=gen) - 0.4
    noise_a = torch.empty(2 ** 29, dtype=torch.float32, device=dev)        # 2 GiB
    noise_b = torch.empty_like(noise_a)
    side = torch.cuda.Stream()
    ref = None
    for it in range(12):
        if it % 2:
            with torch.cuda.stream(side):
                for _ in range(6):
                    noise_b.copy_(noise_a)
        eng.render_train(geom, tM0)
        g = eng.render_bwd_tape(geom, tM0, d).clone()
        torch.cuda.synchronize()
        if ref is None:
            ref = g
        assert torch.equal(g, ref), (it, float((g - ref).abs().max()))
