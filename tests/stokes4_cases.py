"""The cases of the four-Stokes-plane tests (test_gpu_stokes4, and test_stokes4_cases_cpu, which proves on the CPU that their bounds
see a slip in the fourth plane): the case table, the outputs of mlp_reference.Reference with the mutants built in, the comparator
and the bounds.  NumPy and torch on the CPU only (no CUDA call, at import or later); no test here.

S sets sizes and offsets in the kernels, and at S = 4 (bhn_geom.S <= 4, RaySum::SMAX) they are at their extremes: the ray-sum scratch
in LDS is [NW][Sx][32] with the segment counts behind it at an Sx-dependent offset (fused_common.h RaySum::put / combine, shared by
the 4-, 8- and 12-wave kernels and the general path), every backward forms dE = sum_s dimages[(b Sx + s) R + ray] w[s P + p], the
frame-chunked launch offsets dimages by b0 Sx R, and every LDS plan adds RaySum<NW>::bytes(Sx) = NW (132 + 128 Sx): 2,576 / 5,152 /
7,728 bytes for 4 / 8 / 12 waves at Sx = 4.  LDS bytes below are derived from fused_bwd.hip bwd_plan and general_mlp.hip gen_lds /
gen_lds16 at Sx = 4, against the 163,840 bytes a workgroup can have.

The per-plane image figure: max |img_s - ref_s| / max ref_abs_s, ref_abs the float64 oracle's image of the same problem rendered
with |J| (standalone_cases' convention for signed scatter sums; a quantity of the reference alone; for plane 0, J_0 = I > 0, it is
the figure the suite uses everywhere).  Plane V peaks at 6 to 15 % of plane I: an error over the whole image's maximum measures a
wrong V plane at a fraction of its size.

Mutants (MUTANTS) are built into the reference, float64 oracle or bf16 emulator alike: the emission does not depend on J or on
dimages, so one forward of a reference serves the faithful result and every mutant.
"""
import numpy as np
import torch

from conftest import mask_tie_points
from buffer_contract_cases import RAY_SETS as BC_RAY_SETS
from frame_chunk_cases import RAY_SETS, DENSE, build_problem
from mlp_bounds import (CAPS, GTOL, IMG_TOL, L2TOL, OBSERVED, STOKES4_SHAPES, capped_bounds, caps_of, expected_recipe, kernel_width, l2err,
                        maxerr, problem_class, tensor_l2)
from mlp_problems import f32r, random_problem_inputs, t64, tensor_cuts, without_samples
from mlp_reference import dropped, point_reference
from oracle import oracle_np as onp

S = 4

MUTANTS = {
    'drop_plane3': 'J[3] = 0 and the V residual removed from the loss: a kernel whose plane loops stop at three',
    'plane3_reads_plane2': 'J[3] = J[2]: the fourth weight plane read at the third one\'s offset',
    'dimages_plane3_ignored': 'the gradient with dimages[:, 3] = 0: a backward that sums dE over three planes (images right)',
    'plane_stride_3': 'dimages and images indexed as if Sx were 3: plane s of frame b taken at 3 b + s',
}

# why a shape of mlp_bounds.STOKES4_SHAPES is there (training forward / delta chain / dW kernel LDS bytes at Sx = 4)
SHAPE_WHY = {
    (128, 4, 4, 3): 'fused128: resident 8-wave training forward 150,688 B (bwd_plan res_fwd less the chain rows), bwd128_kernel',
    (256, 4, 4, 3): 'ga0_chain: training forward 158,880 B (EncBlock ring), delta chain with its dW_0 staging images 157,984 B',
    (256, 8, 4, 3): 'the two tightest plans: f32 training forward 162,448 B and delta chain (lds_taped) 163,600 B, 240 B left; bf16 '
                    'training forward 162,976 B -- 164,128 B, 288 B over, while it kept room for the chain\'s zero row and W_out -- and '
                    'ga0_chain delta chain 162,080 B, 1,760 B left',
    (64, 6, 4, 3): 'fold (drop_ga), resident training forward and resident delta chain (ResidentRing: no ring barrier behind the combine)',
    (32, 3, 4, 3): 'the narrowest kernel: MT = 1, skip-concat into layer 2 and into the output layer',
    (256, 2, 4, 3): 'generic tape backward, no W_out fold, at the ga0_chain width',
    (288, 4, 4, 3): 'general path, four groups per workgroup at the LDS ceiling: gen_lds16(Wp 288, Ep 32, ng 4) = 162,336 B, 1,504 B left; '
                    'f32 gen_lds 85,280 B',
    (512, 4, 4, 6): 'general path, the widest: Ep 64; gen_lds(512, 64) = 146,720 B (f32), gen_lds16(512, 64, ng 2) = 145,184 B',
}

X12 = (32, 32, 96, DENSE)         # 3,072 groups per frame: 12-wave tiles (bhn_fwd_tile_groups); G = 96: no direct layout, the LDS combine
SPAN2 = dict(H=48, W=48, G=100, fov=40.0, inc=12.0, seed=3, dom=(20.0, 6.0, 20.0, 4.0), B=2)   # test_gpu_forward's ray_span <= 2 set


# The shell-domain sets (the random problems' 9 x 7 rays x 50 samples, 'compacted', 'span2') keep every ray's in-domain points within two
# 32-point groups (bhn_geom.ray_span = 2), and 'dense 96' has G = 32: on all of them the waves add their ray segments straight to the
# pixels (ray_direct) and the ray-sum scratch in LDS is never touched.  The combine through LDS -- the [NW][Sx][32] scratch with the
# segment counts behind it -- runs on dense rays of 50 or 96 samples: 'ragged' (buffer_contract_cases: 37 rays x 50 samples, 58
# groups, the last one 26 points) on the 4-wave (f32), 8-wave (bf16) and general-path kernels, 'x12' on the 12-wave one.
def _chi2(width, depth, deg, dt='full'):
    return dict(kind='chi2', width=width, depth=depth, deg=deg, dt=dt, modes=('f32', 'bf16'), general=width > 256 or deg > 4, compact=True,
                direct=True, why=SHAPE_WHY[(width, depth, S, deg)] + ('' if dt == 'full' else "; 'lc': chi2_image sums B Sx light curves"))


def _linear(width, depth, modes, rays, why, B=3, routes_bitwise=False, **kw):
    return dict(kind='linear', width=width, depth=depth, deg=3, modes=modes, general=width > 256, rays=rays, B=B, routes_bitwise=routes_bitwise,
                compact=rays in ('compacted', 'span2'), direct=rays not in ('ragged', 'x12'), why=why, **kw)


CASES = {'%dx%d S4 deg%d' % (d, w, deg): _chi2(w, d, deg) for w, d, _, deg in STOKES4_SHAPES}
CASES.update({
    '4x128 S4 deg3 lc': _chi2(128, 4, 3, 'lc'),
    # direct ray sums: G = 32 rays start on group boundaries, every wave adds its segments straight to the pixels (RaySum::direct /
    # put with ray_direct), four atomics per segment; render == render_train and recompute == recorded tape bit for bit
    '4x128 S4 dense 96': _linear(128, 4, ('bf16',), 'dense 96', 'ray_direct, fused128', routes_bitwise=True),
    '4x256 f32 S4 dense 96': _linear(256, 4, ('f32',), 'dense 96', 'ray_direct, f32 4-wave kernels (RaySum<4>): training forward and '
                                     'delta chain 158,352 / 159,504 B', routes_bitwise=True),
    '4x128 S4 compacted': _linear(128, 4, ('bf16',), 'compacted', 'point-compacted shell (ray_idx), 18 x 15 rays: ray_span 2, direct adds'),
    '4x64 f32 S4 compacted': _linear(64, 4, ('f32',), 'compacted', 'point-compacted shell on the f32 kernels: ray_span 2, direct adds'),
    '4x128 S4 span2': _linear(128, 4, ('bf16',), 'span2', 'compacted rays within two groups (bhn_geom.ray_span <= 2) at 2,304 rays: the '
                              'combine is skipped, every wave adds four planes per segment', B=SPAN2['B']),
    '4x128 S4 x12': _linear(128, 4, ('bf16',), 'x12', '12-wave tiles WITH the LDS combine: resident 12-wave training forward 153,264 B '
                            '(RaySum<12> 7,728 B), the largest ray-sum scratch', B=2, tile_groups=12),
    # the LDS combine at four planes on every other kernel family, the tightest plans among them WITH their scratch in use
    '4x256 S4 ragged': _linear(256, 4, ('bf16',), 'ragged', 'LDS combine, 8-wave ring kernels (RaySum<8> 5,152 B): ga0_chain'),
    '8x256 S4 ragged': _linear(256, 8, ('f32', 'bf16'), 'ragged', 'LDS combine in the two tightest plans: f32 162,448 / 163,600 B '
                               '(RaySum<4> 2,576 B ends 240 B under the limit in the delta chain), bf16 training forward 162,976 B'),
    '6x64 S4 ragged': _linear(64, 6, ('f32', 'bf16'), 'ragged', 'LDS combine in the resident kernels (ResidentRing: the barrier behind '
                              'the combine is the kernel\'s own), 8 waves and (f32) 4 waves'),
    '4x288 S4 ragged': _linear(288, 4, ('f32', 'bf16'), 'ragged', 'LDS combine on the general path (RaySum<GEN_TG>): bf16 four groups per '
                               'workgroup, 162,336 B, the scratch ends 1,504 B under the limit'),
})


def case_recipe(name, mode):
    c = CASES[name]
    return expected_recipe(c['depth'], kernel_width(c['width']), c['general']) if mode == 'bf16' else None


# ---- the problems
_PROBLEMS = {}


def _span2_problem(c):
    """test_gpu_forward.test_compacted_rays_within_two_groups_skip_the_combine's ray set (48 x 48 rays x 100 samples, inclination 12
    degrees, domain r 6 .. 20, |z| <= 4) with a V row, a network of its own and two frames."""
    from bhnerf_amd import synthetic
    sp = SPAN2
    geo = synthetic.synthetic_geodesics(sp['H'], sp['W'], sp['G'], fov_M=sp['fov'], inc_deg=sp['inc'], spin=0.0, S=3, seed=sp['seed'])
    rng = np.random.default_rng(4004)
    g = {k: f32r(geo[k]) for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    J3 = f32r(geo['J'])
    g['J'] = np.concatenate([J3, f32r(J3[:1] * rng.uniform(-0.5, 0.5, J3[:1].shape))])
    depth, width = c['depth'], c['width']
    tree = onp.he_uniform_params(rng, depth, width, 21, dtype=np.float32)
    for i in range(depth + 1):
        g['kernel%d' % i] = tree['MLP_0']['Dense_%d' % i]['kernel'].astype(np.float64)
        g['bias%d' % i] = f32r(rng.uniform(-0.1, 0.1, tree['MLP_0']['Dense_%d' % i]['bias'].shape))
    g['bias%d' % depth] = g['bias%d' % depth] + 9.0
    B = sp['B']
    g.update(t_frames=np.linspace(0.0, 1.5, 5)[:B], t_start_obs=0.0, t_injection=float(geo['t_injection']),
             hparams=np.array(list(sp['dom']) + [3, depth, width, 1.0]))
    # a sample whose domain mask is decided within f32 rounding leaves the problem on both sides (Doppler weight 0)
    g = without_samples(g, mask_tie_points(g).any(axis=0))
    gen = torch.Generator().manual_seed(4005)
    dimg = (torch.rand((B, S, sp['H'] * sp['W']), generator=gen, dtype=torch.float64) - 0.4).float().double()
    return dict(g=g, dimg=dimg, spatial=(sp['H'], sp['W']))


def problem(name):
    """The problem of a case: g (g5 layout, float64 arrays of f32-rounded values, J (4, H, W, G)), spatial, and 'linear': dimg
    (B, 4, R), different in every frame and plane; 'chi2': target, sigma, offset."""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    c = CASES[name]
    if c['kind'] == 'chi2':
        p = random_problem_inputs(c['width'], c['depth'], S, c['deg'])
        prob = dict(g=p['g'], spatial=p['g']['coords'].shape[1:3], target=p['target'], sigma=p['sigma'], offset=p['offset'])
        if c['dt'] == 'lc':
            # test_gpu_fullsize_stokes' well-conditioned light-curve chi^2: residuals of 40 to 70 %, one noise level per problem
            lc0 = reference(name, None, prob=prob).images().sum(dim=(-1, -2)).numpy()
            rng = np.random.default_rng(4001)
            prob.update(target=lc0 * rng.uniform(0.3, 0.6, lc0.shape), sigma=np.abs(lc0[:, :1]).mean() * rng.uniform(0.05, 0.2, lc0.shape),
                        offset=np.zeros_like(lc0))
    elif c['rays'] == 'span2':
        prob = _span2_problem(c)
    else:
        H, Wd, G, dom = X12 if c['rays'] == 'x12' else BC_RAY_SETS['ragged'] if c['rays'] == 'ragged' else RAY_SETS[c['rays']]
        p = build_problem(c['depth'], c['width'], c['modes'][0], S, 3, H, Wd, G, dom, c['B'])
        prob = dict(g=p['g'], dimg=p['dimg'], spatial=p['spatial'])
    assert prob['g']['J'].shape[0] == S
    _PROBLEMS[name] = prob
    return prob


def three_planes(g):
    """The problem with the V row removed."""
    return dict(g, J=g['J'][:3])


# ---- the references (mlp_reference.Reference: the emission once on the in-domain points, images and gradient for any J)
def reference(name, recipe, drop=None, prob=None):
    """The Reference of a case, made once (`prob`: while problem() builds it)."""
    return point_reference('stokes4', name, problem(name) if prob is None else prob, recipe, drop)


def stride3(x):
    """x (B, 4, ...) as a kernel reads it that takes plane s of frame b at 3 b + s."""
    B = x.shape[0]
    idx = torch.tensor([3 * b + s for b in range(B) for s in range(S)])
    return x.reshape((B * S,) + tuple(x.shape[2:]))[idx].reshape(x.shape)


def chi2_dimages(images, prob, dt):
    """d chi^2 / d images (oracle_torch.loss_image, loss scale 1)."""
    tg, sg, of = (t64(prob[k]) for k in ('target', 'sigma', 'offset'))
    if dt == 'full':
        return 2.0 * (images - tg - of) / sg ** 2
    return (2.0 * (images.sum(dim=(-1, -2)) - tg - of) / sg ** 2)[..., None, None].expand_as(images).contiguous()


def outputs(name, ref, prob, mutant=None):
    """What the case compares, from a Reference: images (B, 4, R) and the flat gradient -- 'linear': of sum(images dimg), 'chi2': of the
    chi^2 of the case's targets -- with the slip `mutant` built in."""
    assert mutant is None or mutant in MUTANTS
    c = CASES[name]
    J = ref.J
    if mutant == 'drop_plane3':
        J = J.clone(); J[3] = 0.0
    elif mutant == 'plane3_reads_plane2':
        J = J.clone(); J[3] = J[2]
    img = ref.images(J)
    dimg = prob['dimg'].reshape(img.shape) if c['kind'] == 'linear' else chi2_dimages(img, prob, c['dt'])
    if mutant in ('drop_plane3', 'dimages_plane3_ignored'):
        dimg = dimg.clone(); dimg[:, 3] = 0.0
    elif mutant == 'plane_stride_3':
        img, dimg = stride3(img), stride3(dimg)
    return dict(images=img.numpy().reshape(img.shape[0], S, -1), grad=ref.grad(dimg, J))


def fits(name, mutant):
    """Whether a case must see a mutant.  dimages_plane3_ignored is a slip of the LINEAR gradient (bhn_render_bwd's dimages); in a
    chi^2 case it is drop_plane3 with the images left right -- its gradient alone, 8e-3 of the 6x64 problem's, is 2.6x the
    emulator cap there, so it is printed and not required."""
    return mutant != 'dimages_plane3_ignored' or CASES[name]['kind'] == 'linear'


# ---- the comparator
def plane_figures(images, ref_images, ref_abs):
    """Per plane: max |img_s - ref_s| / max ref_abs_s over frames and rays; images (B, 4, R)."""
    return [float(np.abs(images[:, s] - ref_images[:, s]).max() / ref_abs[:, s].max()) for s in range(S)]


def figures(out, ref64, ref_abs, cuts, emu=None):
    """The figures of one run `out` (outputs' layout): against the float64 oracle `ref64` -- planes, gmax, grad (relative L2) -- and,
    for a bf16 run, against the emulator `emu` -- em_image (whole image), em_grad, em_tensor (worst kernel / bias tensor)."""
    f = dict(planes=plane_figures(out['images'], ref64['images'], ref_abs), gmax=maxerr(out['grad'], ref64['grad']), grad=l2err(out['grad'], ref64['grad']))
    if emu is not None:
        f.update(em_image=maxerr(out['images'], emu['images']), em_grad=l2err(out['grad'], emu['grad']),
                 em_tensor=max(tensor_l2(out['grad'], emu['grad'], cuts, True)))
    return f


def bounds(name, mode):
    """The bounds of a case.  f32: IMG_TOL per plane, GTOL / L2TOL.  bf16: against the float64 oracle IMG_TOL['bf16'] per plane;
    against the emulator 4x the case's own figures (mlp_bounds.OBSERVED; a case not yet measured: the caps), never above the caps of
    its class -- 'fused128' for 4x128, else 'random'.  Class 'deep' (8x256) has no cap: the bf16 mode's GTOL / L2TOL against the
    oracle, and against the emulator never above 4x the figures of the same network at three planes, OBSERVED['8x256 S3 deg3']
    (1.4e-3 image, 3.3e-3 gradient, 1.1e-2 worst tensor)."""
    c = CASES[name]
    b = dict(planes=IMG_TOL[mode], gmax=GTOL[mode], grad=L2TOL[mode])
    if mode == 'bf16':
        keys = ('image', 'grad', 'tensor')
        if problem_class(c['depth'], c['width']) == 'deep':
            o = OBSERVED['8x256 S3 deg3']
            caps = capped_bounds(keys, (o[0], o[3], o[4]), {})
        else:
            # the gradient is held to the emulator, 20x closer than the bf16 quantisation noise lets the float64 oracle hold it
            # (posenc degree 6: the emulator itself is 7.1e-2 from the oracle, over L2TOL)
            del b['gmax'], b['grad']
            caps = caps_of('fused128' if (c['depth'], kernel_width(c['width'])) == (4, 128) and not c['general'] else 'random', c['deg'])
            assert set(caps) == set(CAPS['random'])
        o = OBSERVED.get(name)
        eb = caps if o is None else capped_bounds(keys, (o[0], o[3], o[4]), caps)
        b.update(em_image=eb['image'], em_grad=eb['grad'], em_tensor=eb['tensor'])
    return b


def ratios(fig, b):
    """{figure: figure / bound}; the planes one by one."""
    r = {'plane%d' % s: v / b['planes'] for s, v in enumerate(fig['planes'])}
    r.update({k: fig[k] / b[k] for k in b if k != 'planes'})
    return r


def within(fig, b):
    return all(v < 1.0 for v in ratios(fig, b).values())


def describe(fig):
    s = 'planes %s  gradient max %.2e L2 %.2e' % (' '.join('%.2e' % v for v in fig['planes']), fig['gmax'], fig['grad'])
    if 'em_grad' in fig:
        s += '  vs emulator: image %.2e gradient %.2e worst tensor %.2e' % (fig['em_image'], fig['em_grad'], fig['em_tensor'])
    return s


def case_references(name, mode, drop=None):
    """(prob, ref64 outputs, ref_abs, emulator outputs or None, cuts, the two References) of a case in a mode."""
    prob = dropped(problem(name), drop)
    r64 = reference(name, None, drop)
    recipe = case_recipe(name, mode)
    rem = None if recipe is None else reference(name, recipe, drop)
    ref_abs = r64.images(r64.J.abs()).numpy().reshape(len(prob['g']['t_frames']), S, -1)
    assert (ref_abs.reshape(-1, S, ref_abs.shape[-1]).max(axis=(0, 2)) > 0).all()
    return dict(prob=prob, ref64=outputs(name, r64, prob), ref_abs=ref_abs, emu=None if rem is None else outputs(name, rem, prob),
                cuts=tensor_cuts(prob['g'], CASES[name]['depth']), r64=r64, rem=rem)
