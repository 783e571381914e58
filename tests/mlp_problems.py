"""The problems of the MLP kernel tests and their float64 references, each written once: the tilted ray grid behind random_problem and
frame_chunk_cases.build_problem, the oracle's inputs from a problem in the layout of a g5_* fixture, the chi^2 targets, the flat
gradient in flax tree order, the tie adjudication's dropped samples, the small problem of the identity tests and the config-scale
problem of the full-size tests.  CPU only (no CUDA call, at import or later); no test here.  tests/test_mlp_problems_cpu.py pins what
the builders draw by sha256."""
import hashlib

import numpy as np
import torch

from conftest import golden_tree, relu_tie_count
from oracle import oracle_np as onp
from oracle import oracle_torch as ot

RANDOM_PROBLEM_SHAPE = (9, 7, 50, 3)       # rays H x W, samples per ray, frames of random_problem (tools/fuzz_parity.py varies it)
RANDOM_PROBLEM_DOMAIN = (8.0, 2.5, 8.0, 4.0)   # scale, rmin, rmax, z_width of the recovery domain (fuzz: random)
RANDOM_PROBLEM_JITTER = (0.0, 0.0, 0.0)    # offsets of the alpha / beta / sample grids: regular grids of other shapes put samples EXACTLY
                                           # on the domain boundary (e.g. 10 x 7 rays x 64 samples: alpha^2 + beta^2 + s^2 = rmax^2),
                                           # where the f32 kernel and the f64 oracle legitimately disagree about the mask


def f32r(v):
    """float32-rounded values held as float64: identical inputs on both sides, the oracle evaluates them in float64."""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def f32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


def t64(x):
    return torch.tensor(np.asarray(x, dtype=np.float64))


def tilted_ray_grid(H, W, G, jitter=(0.0, 0.0, 0.0)):
    """H x W rays of G samples through the origin at 60 degrees inclination: (dict of coords (3, H, W, G), Omega = 1 / (r^1.5 + 0.1),
    t_geos = -(1000 - (s + 9.6)), Sigma, dtau -- float64, not yet rounded, without the Doppler weight g, which the caller draws --, r)."""
    ja, jb, js = jitter
    alpha, beta = np.meshgrid(np.linspace(-8 + ja, 8 + ja, H), np.linspace(-8 + jb, 8 + jb, W), indexing='ij')
    s = np.linspace(-9.6 + js, 9.6 + js, G)
    inc = np.deg2rad(60.0)
    coords = np.stack([alpha[..., None] * np.ones(G), beta[..., None] * np.cos(inc) + s * np.sin(inc),
                       -beta[..., None] * np.sin(inc) + s * np.cos(inc)])
    r = np.sqrt((coords ** 2).sum(0)) + 0.3
    return dict(coords=coords, Omega=1.0 / (r ** 1.5 + 0.1), t_geos=-(1000.0 - (s + 9.6)) * np.ones_like(r), Sigma=r ** 2,
                dtau=(s[1] - s[0]) / r ** 2), r


def stokes_factors(rng, shape, S):
    """J (S, *shape), 0 < S <= 4 (bhn_geom.S <= 4; anything else raises): I and chi are drawn whatever S is, so the draws that follow
    do not depend on S <= 3; the circular row V = I U(-0.5, 0.5) is drawn after them and only for S = 4.  Linear fraction 0.85:
    Q^2 + U^2 + V^2 <= (0.85^2 + 0.5^2) I^2 = 0.9725 I^2."""
    if not 0 < S <= 4:
        raise ValueError('stokes_factors: S = %r, the kernels take 1 .. 4 Stokes planes' % (S,))
    I = rng.uniform(0.5, 1.5, shape); chi = rng.uniform(0, np.pi, shape)
    rows = [I, 0.85 * I * np.cos(2 * chi), 0.85 * I * np.sin(2 * chi)][:S]
    if S == 4:
        rows.append(I * rng.uniform(-0.5, 0.5, shape))
    J = np.stack(rows)
    assert J.shape[0] == S
    return J


def oracle_inputs_of(tree, geo, t_injection, dom, deg, depth, do_skip=None, t_start_obs=0.0, GM_c3=onp.GM_C3_SGRA_HR, dtype=torch.float64):
    """(ks, bs, geom, hp) for ot.CpuTrainer / ob.Bf16Trainer / ot.grad_linear from a parameter tree, a geometry dict of float64 arrays
    (J: (S, H, W, G), or None / absent / a 0-d array for none) and the recovery domain (scale, rmin, rmax, z_width)."""
    ks, bs = ot.tree_to_lists(tree, dtype)
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float64), dtype=dtype)
    J = geo.get('J')
    geom = {k: t(geo[k]) for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    geom.update(J=None if J is None or not np.ndim(J) else t(J), t_start_obs=float(t_start_obs), t_injection=float(t_injection))
    scale, rmin, rmax, z_width = (float(v) for v in dom)
    hp = dict(GM_c3=GM_c3, scale=scale, rmin=rmin, rmax=rmax, z_width=z_width, posenc_deg=int(deg), net_depth=int(depth))
    if do_skip is not None:
        hp['do_skip'] = do_skip
    return ks, bs, geom, hp


def oracle_inputs(g, dtype=torch.float64):
    """oracle_inputs_of a problem in the layout of a g5_* fixture (kernel<i>, bias<i>, the geometry arrays, J 0-d when there is none,
    t_start_obs, t_injection, hparams = scale, rmin, rmax, z_width, posenc degree, depth, width, loss scale)."""
    hp = g['hparams']
    return oracle_inputs_of(golden_tree(g), g, g['t_injection'], hp[:4], hp[4], hp[5], t_start_obs=g['t_start_obs'], dtype=dtype)


def oracle_trainer(g, dtype=torch.float64, **kw):
    """(ot.CpuTrainer of a g5-layout problem, the tensor constructor for its arguments)."""
    return ot.CpuTrainer(*oracle_inputs(g, dtype), **kw), lambda x: torch.tensor(x, dtype=dtype)


def flat_grad(grads):
    """CpuTrainer.loss_and_grad's gradients (kernels, then biases) as one float64 array in flax tree order: kernel_0, bias_0, kernel_1, ..."""
    n = len(grads) // 2
    return np.concatenate([np.concatenate([grads[i].numpy().ravel(), grads[n + i].numpy().ravel()]) for i in range(n)])


def targets(g, dt):
    S = g['J'].shape[0] if g['J'].ndim else None
    b = len(g['t_frames'])
    sp = g['coords'].shape[1:3]
    if dt == 'full':
        shape = (b, S) + sp if S else (b,) + sp
    else:
        shape = (b, S) if S else (b,)
    return {k: g[k + '_' + dt].reshape(shape) for k in ('target', 'sigma', 'offset')}


def tensor_cuts(g, depth=None):
    """Offsets of kernel_0, bias_0, kernel_1, ... in the flat flax-order parameter vector of a g5-layout problem."""
    depth = int(g['hparams'][5]) if depth is None else depth
    return np.cumsum([0] + [g[k % i].size for i in range(depth + 1) for k in ('kernel%d', 'bias%d')])


def without_samples(g, drop):
    """The g5-layout problem without the ray samples `drop` (H, W, G) bool: Doppler weight 0 on both sides, so they no longer reach the
    image (the ReLU-tie adjudication); `drop` None: the problem itself."""
    return g if drop is None else dict(g, g=np.where(drop, 0.0, g['g']))


def problem_checksum(prob):
    """sha256 (first 16 hex digits) of a frame_chunk_cases.build_problem dict: what the CPU tests of the case tables pin."""
    h = hashlib.sha256()
    for k in sorted(prob['g']):
        a = np.ascontiguousarray(np.asarray(prob['g'][k], dtype=np.float64))
        h.update(k.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    d = prob['dimg'].numpy()
    h.update(repr((d.shape, prob['dom'], prob['depth'], prob['width'], prob['S'], prob['B'], prob['spatial'])).encode())
    h.update(np.ascontiguousarray(d).tobytes())
    return h.hexdigest()[:16]


def random_problem_inputs(width, depth, S, deg, nudge=0.0, drop_ties=False, shape=RANDOM_PROBLEM_SHAPE, domain=RANDOM_PROBLEM_DOMAIN,
                          jitter=RANDOM_PROBLEM_JITTER, do_skip=True):
    """random_problem without its float64 reference.  do_skip False: the network without skip connections (its layers draw other
    shapes; conftest.relu_tie_count walks the skip network, so no ties are counted and none can be dropped)."""
    assert do_skip or not drop_ties
    rng = np.random.default_rng(width + depth)
    H, Wd, G, B = shape
    geo, r = tilted_ray_grid(H, Wd, G, jitter)
    geo['g'] = rng.uniform(0.6, 1.4, r.shape)
    J = stokes_factors(rng, r.shape, S) if S else None
    t_frames = np.sort(rng.uniform(0, 1, B)); t_inj = -(1000.0 - 4.0)
    geo = {k: f32r(v) for k, v in geo.items()}
    J = f32r(J) if S else None
    tree = onp.he_uniform_params(rng, depth, width, 3 + 6 * deg, do_skip=do_skip, dtype=np.float32)
    nrng = np.random.default_rng(977)
    for i in range(depth + 1):
        d = tree['MLP_0']['Dense_%d' % i]
        d['kernel'] = d['kernel'].astype(np.float64)
        d['bias'] = f32r(rng.uniform(-0.1, 0.1, d['bias'].shape))
        if nudge:                            # tie adjudication: every weight moved by a random relative amount <= nudge
            d['kernel'] = f32r(d['kernel'] * (1.0 + nudge * nrng.uniform(-1, 1, d['kernel'].shape)))
            d['bias'] = f32r(d['bias'] * (1.0 + nudge * nrng.uniform(-1, 1, d['bias'].shape)))
    g = dict(geo, J=(J if S else np.array(1.0)), t_frames=t_frames, t_start_obs=0.0, t_injection=t_inj,
             hparams=np.array(list(domain) + [deg, depth, width, 1.0]))
    for i in range(depth + 1):
        g['kernel%d' % i] = tree['MLP_0']['Dense_%d' % i]['kernel']; g['bias%d' % i] = tree['MLP_0']['Dense_%d' % i]['bias']
    ties, tied = relu_tie_count(g, return_points=True) if do_skip else (0, None)
    dropped, ties_left = 0, ties
    if drop_ties:                            # tie adjudication: the tied ray samples no longer reach the image
        g = without_samples(g, tied)
        dropped = int(tied.sum())
        # re-run the detection on the MODIFIED problem: tied samples that still reach the image (Doppler weight != 0)
        _, tied2 = relu_tie_count(g, return_points=True)
        ties_left = int((tied2 & (np.broadcast_to(g['g'], tied2.shape) != 0)).sum())
    tshape = (B, S, H, Wd) if S else (B, H, Wd)
    target = rng.uniform(0, 1e-3, tshape); sigma = rng.uniform(0.5, 2.0, tshape); offset = np.zeros(tshape)
    return dict(g=g, S=S, t_frames=t_frames, t_inj=t_inj, target=target, sigma=sigma, offset=offset, ties=ties, dropped=dropped,
                ties_left=ties_left)


def random_problem(width, depth, S, deg, nudge=0.0, drop_ties=False, shape=RANDOM_PROBLEM_SHAPE, domain=RANDOM_PROBLEM_DOMAIN,
                   jitter=RANDOM_PROBLEM_JITTER):
    """A ragged problem in g5 layout on the tilted ray grid (`shape`: rays H x W, samples, frames; G = 50 rays straddle wave tiles,
    several workgroup tiles, pre-injection and out-of-domain samples) with its float64 reference images and gradient.  Everything is
    rounded to float32 first, the oracle then evaluates those values in float64.  nudge / drop_ties: the two tie adjudications."""
    prob = random_problem_inputs(width, depth, S, deg, nudge, drop_ties, shape, domain, jitter)
    tr, t = oracle_trainer(prob['g'])
    _, img_ref, grads_ref = tr.loss_and_grad(t(prob['t_frames']), t(prob['target']), t(prob['sigma']), t(prob['offset']), 1.0, 'full')
    return dict(prob, img_ref=img_ref, gref=flat_grad(grads_ref))


def random_problem_emulator_args(width, depth, S, deg):
    """random_problem in the terms of ob.Bf16Trainer: (ks, bs, geom, hp, t_frames, [target, sigma, offset])."""
    prob = random_problem_inputs(width, depth, S, deg)
    return oracle_inputs(prob['g']) + (t64(prob['t_frames']), [t64(prob[k]) for k in ('target', 'sigma', 'offset')])


def golden_problem(g, dt):
    """A g5_* fixture in the terms of ob.Bf16Trainer: (ks, bs, geom, hp, t_frames, [target, sigma, offset], loss scale)."""
    tg = targets(g, dt)
    return oracle_inputs(g) + (t64(g['t_frames']), [t64(tg[k]) for k in ('target', 'sigma', 'offset')], float(g['hparams'][7]))


def small_ray_grid():
    """6 x 5 rays x 40 samples: (dict as tilted_ray_grid's, r).  NOT the tilted grid at another size: extent 7 and 9, direction cosines
    0.5 / 0.8 where the tilted grid has cos 60 deg = 0.5000000000000001."""
    alpha, beta = np.meshgrid(np.linspace(-7, 7, 6), np.linspace(-7, 7, 5), indexing='ij')
    s = np.linspace(-9.0, 9.0, 40)
    coords = np.stack([alpha[..., None] * np.ones(40), beta[..., None] * 0.5 + s * 0.8, -beta[..., None] * 0.8 + s * 0.5])
    r = np.sqrt((coords ** 2).sum(0)) + 0.3
    return dict(coords=coords, Omega=1.0 / (r ** 1.5 + 0.1), t_geos=-(1000.0 - (s + 9.0)) * np.ones_like(r), Sigma=r ** 2,
                dtau=(s[1] - s[0]) / r ** 2), r


def small_problem(depth, width, S, do_skip, deg=3, seed=0):
    """A small random problem (small_ray_grid, 2 frames, masked domain) for the identity tests of the bf16 emulator, in the emulator's
    terms.  Its biases are float32, not rounded through float64 as random_problem's, so it stays a builder of its own."""
    rng = np.random.default_rng(seed + 10 * depth + S)
    B = 2
    geo, r = small_ray_grid()
    H, Wd, _ = r.shape
    tr = lambda v: torch.tensor(f32r(v))
    geom = {k: tr(v) for k, v in dict(geo, g=rng.uniform(0.6, 1.4, r.shape)).items()}
    geom.update(t_start_obs=0.0, t_injection=-(1000.0 - 3.0), J=tr(stokes_factors(rng, r.shape, S)) if S else None)
    tree = onp.he_uniform_params(rng, depth, width, 3 + 6 * deg, do_skip=do_skip, dtype=np.float32)
    for i in range(depth + 1):
        d = tree['MLP_0']['Dense_%d' % i]
        d['bias'] = rng.uniform(-0.1, 0.1, d['bias'].shape).astype(np.float32)
    tree['MLP_0']['Dense_%d' % depth]['bias'] = tree['MLP_0']['Dense_%d' % depth]['bias'] + 9.0
    ks, bs = ot.tree_to_lists(tree)
    hp = dict(GM_c3=onp.GM_C3_SGRA_HR, scale=8.0, rmin=2.0, rmax=8.0, z_width=4.0, posenc_deg=deg, net_depth=depth, do_skip=do_skip)
    shape = (B, S, H, Wd) if S else (B, H, Wd)
    tg = [torch.tensor(rng.uniform(0, 1e-2, shape)), torch.tensor(rng.uniform(0.5, 2.0, shape)), torch.zeros(shape, dtype=torch.float64)]
    return ks, bs, geom, hp, torch.tensor(np.linspace(0.1, 0.7, B)), tg


# ---- the config-scale problems of the full-size tests
def config_tree(rng, width):
    """The 4 x width network of the full-size tests: He-uniform kernels, biases from U(-0.05, 0.05), output bias + 9 (emission ~
    sigmoid(-1): a visible image), float32."""
    tree = onp.he_uniform_params(rng, 4, width, 21, dtype=np.float32)
    for i in range(5):
        d = tree['MLP_0']['Dense_%d' % i]
        d['bias'] = rng.uniform(-0.05, 0.05, d['bias'].shape).astype(np.float32)
    tree['MLP_0']['Dense_4']['bias'] = tree['MLP_0']['Dense_4']['bias'] + 9.0
    return tree


def config_problem(H, W, G, width, fov, inc, spin, S, seeds, t_frames):
    """A BASELINE-config-sized problem: synthetic geodesics (seeds[0]) and config_tree (seeds[1]).  The caller adds what needs a device."""
    from bhnerf_amd import constants, synthetic
    geo = synthetic.synthetic_geodesics(H, W, G, fov_M=fov, inc_deg=inc, spin=spin, S=S, seed=seeds[0])
    return dict(geo=geo, t_frames=t_frames, tree=config_tree(np.random.default_rng(seeds[1]), width), GM_c3=constants.GM_c3('hr'))


# BASELINE config 2 (128 x 128 rays x 64 samples, 8 frames per step, 4x256) on its two recovery domains, and the polarised configs 3 and 5
CONFIG2 = dict(H=128, W=128, G=64, width=256, fov=16.0, inc=60.0, spin=0.0, S=0, seeds=(0, 5), t_frames=np.linspace(0.0, 1.0, 64)[:8])
CONFIG2_DOMAINS = {'masked': (8.0, 2.0, 8.0, 4.0),                    # scale, rmin, rmax, z_width: tutorial-style recovery domain
                   'all_active': (8.0, 0.0, np.inf, np.inf)}          # bench.py's headline variant
STOKES_CONFIGS = {
    'config3': dict(H=256, W=256, G=128, width=256, fov=40.0, inc=60.0, spin=0.94, rmin=2.024, rmax=20.0, z_width=4.0),
    'config5': dict(H=64, W=64, G=100, width=128, fov=40.0, inc=12.0, spin=0.0, rmin=6.0, rmax=20.0, z_width=4.0),
}


def stokes_problem(name):
    """config_problem of a polarised config (S = 3, 8 frames) + its table entry `c`."""
    c = STOKES_CONFIGS[name]
    p = config_problem(c['H'], c['W'], c['G'], c['width'], c['fov'], c['inc'], c['spin'], 3, (3, 21), np.linspace(0.0, 1.7, 128)[:8])
    return dict(p, c=c)


def stokes_domain(c):
    return (c['rmax'], c['rmin'], c['rmax'], c['z_width'])


def rays_through_domain(geo, c, seed, n=256):
    """n rays, sorted, drawn among those with at least four samples inside the recovery domain of `c` (most rays of a 40 M field of view
    miss |z| <= 4, r <= 20)."""
    G = geo['coords'].shape[-1]
    r2 = (geo['coords'] ** 2).sum(0).reshape(-1, G)
    inside = ((r2 >= c['rmin'] ** 2) & (r2 <= c['rmax'] ** 2) & (np.abs(geo['coords'][2].reshape(-1, G)) <= c['z_width'])).sum(1)
    return np.sort(np.random.default_rng(seed).choice(np.nonzero(inside >= 4)[0], size=n, replace=False))


def ray_subset(geo, rays, stokes=False):
    """256 rays of a geometry as a 16 x 16 image plane of their own (rays are independent): contiguous arrays, J (3, ...) or None."""
    G = geo['coords'].shape[-1]
    sub = lambda v: np.ascontiguousarray(v.reshape((-1, G))[rays].reshape(16, 16, G))
    g = {k: sub(geo[k]) for k in ('Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    return dict(g, coords=np.stack([sub(geo['coords'][i]) for i in range(3)]), J=np.stack([sub(geo['J'][s]) for s in range(3)]) if stokes else None)


def oracle_images(p, rays, dom, stokes=False):
    """The float64 numpy oracle's images of the 96 rays `rays` of a config_problem in the domain `dom`: (B, 96), or (B, 3, 96) with J."""
    geo = p['geo']
    G = geo['coords'].shape[-1]
    scale, rmin, rmax, z_width = dom
    # (as a 12 x 8 "image": the reference's squeeze / broadcast conventions, which the oracle keeps, assume no
    #  singleton spatial axis)
    sub = lambda v: v.reshape((-1, G))[rays].reshape(12, 8, G).astype(np.float64)
    coords = np.stack([sub(geo['coords'][i]) for i in range(3)])
    J = np.stack([sub(geo['J'][s]) for s in range(3)]) if stokes else 1.0
    tree = {'MLP_0': {k: {kk: np.asarray(vv, dtype=np.float64) for kk, vv in v.items()} for k, v in p['tree']['MLP_0'].items()}}
    e = onp.predictor_apply(tree, p['t_frames'], coords, sub(geo['Omega']), 0.0, sub(geo['t_geos']), float(geo['t_injection']),
                            GM_c3=p['GM_c3'], scale=scale, rmin=rmin, rmax=rmax, z_width=z_width)
    img = onp.image_plane_prediction(e, J, sub(geo['g']), sub(geo['dtau']), sub(geo['Sigma']))
    return img.reshape((len(p['t_frames']), 3, 96) if stokes else (len(p['t_frames']), 96))
