"""The cases of test_gpu_step_same_bits (held to their rules on the CPU by test_step_cases_cpu): two gradient steps of every training
path but the bf16 width-256 one, which test_gpu_w256_same_bits pins -- each case in the terms of same_bits.run_case, with the path it
must reach (`path`: gpu_support.expected_flags' recipe), the layout it must have (`groups` of 32 points per frame, `compact`,
`tile_groups` of the training forward where the case is about them) and `why` it is there.  Also the reference of a case's FIRST step
(the float64 oracle or the bf16 emulator of the path) and the bounds it is held to, none of which comes from the kernels under
test.  CPU only; no test here.

Ray sets (mlp_problems.tilted_ray_grid; posenc degree 3 unless the case says otherwise):
    RAGGED    37 x 1 rays x 50 samples, all-active: 1850 points = 58 groups, the last one 26 points, 50-sample rays straddle the groups;
              58 = 7 tiles of 8 + 2 = 14 quads of groups + 2
    ROWS[48]  48 x 32 rays x 64 samples, all-active: 3072 groups per frame, the training forward of the fused 4x128 path runs tiles of 12
    ROWS[47]  47 x 32 rays x 64 samples: 3008 groups, tiles of 8 (test_gpu_backward.test_reference_default_network_on_twelve_and_eight_
              group_tiles' two layouts)
    the compacted layout of mlp_problems.RANDOM_PROBLEM_SHAPE / RANDOM_PROBLEM_DOMAIN: 9 x 7 rays x 50 samples in the shell domain,
              645 in-domain points = 21 groups"""
import numpy as np

from general_path_cases import layout as general_layout, skip_inputs
from mlp_bounds import GTOL, L2TOL, caps_of, expected_recipe, kernel_width, l2err, maxerr, problem_class, tensor_l2
from mlp_problems import RANDOM_PROBLEM_DOMAIN, RANDOM_PROBLEM_SHAPE, flat_grad, oracle_inputs, t64, tensor_cuts, without_samples
from mlp_reference import cached, tie_points
from oracle import oracle_bf16 as ob
from oracle import oracle_torch as ot
from same_bits import case_problem, case_targets

ALL_ACTIVE = (8.0, 0.0, np.inf, np.inf)
RAGGED = (37, 1, 50)
ROWS = {48: (48, 32, 64), 47: (47, 32, 64)}


def case(path, mode, depth, width, why, S=0, rays=RAGGED, B=2, domain=ALL_ACTIVE, dt='full', cap=None, deg=3, do_skip=True, groups=58,
         compact=False, tile_groups=None):
    return dict(path=path, mode=mode, depth=depth, width=width, S=S, shape=tuple(rays) + (B,), domain=domain, dt=dt, cap=cap, deg=deg,
                do_skip=do_skip, groups=groups, compact=compact, tile_groups=tile_groups, why=why)


CASES = {
    # ---- bwd128_kernel + reduce128_kernel: bf16, kernel width 128, depth 4
    'f128_full': case('fused128', 'bf16', 4, 128, 'the reference\'s default network at its full width: no padding, 14 quads of groups + 2'),
    'f128_w113_noskip': case('fused128', 'bf16', 4, 113, '15 zero-padded columns, and without the skip connection the skip tile of layer 3 is '
                             'computed and discarded', do_skip=False),
    'f128_w97_s3_lc': case('fused128', 'bf16', 4, 97, '31 zero-padded columns (a whole 32-column block but one), three Stokes planes, the '
                           'light-curve loss', S=3, dt='lc'),
    'f128_rows48': case('fused128', 'bf16', 4, 128, '3072 groups per frame: the forward pair on 12-wave workgroups, tiles of 12 groups',
                        rays=ROWS[48], B=1, groups=3072, tile_groups=12),
    'f128_rows47': case('fused128', 'bf16', 4, 128, '3008 groups per frame: one row under the threshold, tiles of 8 groups', rays=ROWS[47],
                        B=1, groups=3008, tile_groups=8),
    'f128_compact': case('fused128', 'bf16', 4, 128, 'a point-compacted layout, rays of at most two groups, 21 groups = 5 quads + 1',
                         rays=RANDOM_PROBLEM_SHAPE[:3], B=RANDOM_PROBLEM_SHAPE[3], domain=RANDOM_PROBLEM_DOMAIN, groups=21, compact=True),
    'f128_frame_groups': case('fused128', 'bf16', 4, 128, 'three frames on a workspace capped to a tape of two: groups of 2 + 1, the second '
                              'group\'s gradient added to the first\'s', B=3, cap=2),
    # ---- the W_out fold (drop_ga) outside bwd128_kernel and the ga0 chain: bf16, chain_kernel + dw_kernel
    'fold_4x64': case('fold', 'bf16', 4, 64, 'kernel width 64'),
    'fold_5x128': case('fold', 'bf16', 5, 128, 'width 128 at a depth bwd128_supported refuses; odd depth: the output layer takes the skip input'),
    # ---- depth 2 does not fold W_out (common.h bhn_folds_wout): the generic tape backward
    'generic_2x32': case('generic', 'bf16', 2, 32, 'the smallest network: kernel width 32, two hidden layers, gA_1 from the f32 W_out'),
    # ---- the 8-bit tape: the first step calibrates the tape scales (t8_prepare_kernel on a fresh workspace), the second updates them
    't8_4x256': case('t8', 'bf16_t8', 4, 256, 'the 8-bit tape at the headline shape'),
    't8_8x256_s4': case('t8', 'bf16_t8', 8, 256, 'eight layers of tape scales, four Stokes planes: t8_dmax_kernel scans B * 4 * R entries', S=4),
    # ---- the fused f32 kernels
    'f32_4x32': case('f32', 'f32', 4, 32, 'kernel width 32'),
    'f32_4x128': case('f32', 'f32', 4, 128, 'kernel width 128'),
    'f32_4x256': case('f32', 'f32', 4, 256, 'kernel width 256, the largest the f32 kernels\' LDS holds at depth 4'),
    'f32_4x128_s3_lc': case('f32', 'f32', 4, 128, 'three Stokes planes, the light-curve loss', S=3, dt='lc'),
    'f32_4x256_compact': case('f32', 'f32', 4, 256, 'a point-compacted layout', rays=RANDOM_PROBLEM_SHAPE[:3], B=RANDOM_PROBLEM_SHAPE[3],
                              domain=RANDOM_PROBLEM_DOMAIN, groups=21, compact=True),
    # ---- the general path (posenc degree 5 > 4; width 257 > 256), both modes
    'gen_4x160_deg5_f32': case('general f32', 'f32', 4, 160, 'NG 4: four groups per workgroup pass, MTp 5 on four waves', deg=5),
    'gen_4x160_deg5_bf16': case('general', 'bf16', 4, 160, 'NG 4 on the MFMA kernels', deg=5),
    'gen_4x257_deg5_f32': case('general f32', 'f32', 4, 257, 'NG 2, width padded to 288: 31 zero-padded columns', deg=5),
    'gen_4x257_deg5_bf16': case('general', 'bf16', 4, 257, 'NG 2, 31 zero-padded columns on the MFMA kernels', deg=5),
}
# groups per workgroup pass of the general path's bf16 kernels (general_mlp.hip gen_ng16), as general_path_cases.layout restates it
GENERAL_NG = {'gen_4x160_deg5_f32': 4, 'gen_4x160_deg5_bf16': 4, 'gen_4x257_deg5_f32': 2, 'gen_4x257_deg5_bf16': 2}


def general_ng(c):
    return general_layout(c['depth'], c['width'], c['deg'], c['do_skip'], max(c['S'], 1))['NG']


def is_general(c):
    return c.get('width', 256) > 256 or c.get('deg', 3) > 4


def recipe_of(c):
    """The path the library's selection rules give the case (mlp_bounds.expected_recipe), in gpu_support.expected_flags' terms."""
    mode = c.get('mode', 'bf16')
    if mode == 'f32':
        return 'general f32' if is_general(c) else 'f32'
    if mode == 'bf16_t8':
        return 't8'
    return expected_recipe(c['depth'], kernel_width(c.get('width', 256)), is_general(c))


def layout_of(c, prob):
    """(32-point groups per frame, point-compacted) as the engine lays the case out: it compacts a ray set of which less than 0.9 lie
    in the recovery domain."""
    co, (_, rmin, rmax, zw) = prob['g']['coords'], c['domain']
    r2 = (co ** 2).sum(0)
    inside = ~((r2 < rmin ** 2) | (r2 > rmax ** 2) | (np.abs(co[2]) > zw))
    compact = inside.sum() < 0.9 * inside.size
    n = int(inside.sum()) if compact else inside.size
    return (n + 31) // 32, bool(compact)


def check_path(name, eng, geom, groups, flags):
    """same_bits.run_case's check: the case reaches the path and has the layout it is listed for."""
    from gpu_support import assert_path
    c = CASES[name]
    assert_path(name, eng, geom, c['mode'], c['path'], is_general(c), compact=c['compact'], tile_groups=c['tile_groups'])
    assert groups == c['groups'], (name, groups)
    if geom.compact is not None:
        assert geom.compact['ray_span'] <= 2, (name, geom.compact['ray_span'])


def array_sizes(c):
    """{array name: elements} of what same_bits.run_case returns for a case."""
    H, Wd, _, B = c['shape']
    F, w, d = 3 + 6 * c.get('deg', 3), c.get('width', 256), c['depth']
    skip = skip_inputs(d, c.get('do_skip', True))                                    # layer i takes concat[h_i, enc]
    n = sum(((w if i else 0) + (F if i == 0 or skip[i] else 0) + 1) * (w if i < d else 1) for i in range(d + 1))
    return dict(loss=1, images=B * max(c['S'], 1) * H * Wd, grad=n, params=n, adam_m=n, adam_v=n)


# ---- the reference of a case's first step, and its bounds
def reference_kind(c):
    """'f64': the float64 oracle (f32 mode); 'emulator': the bf16 emulator of the path; 't8': the emulator for the images (the 8-bit
    tape's forward is the bf16 mode's) and the float64 oracle for the gradient, by the bf16 mode's bounds, as
    test_gpu_backward.test_tape8_mode_gradient holds it."""
    return {'f32': 'f64', 'bf16': 'emulator', 'bf16_t8': 't8'}[c.get('mode', 'bf16')]


def emulator_recipe(c, recipe):
    return 'fold' if recipe == 't8' else recipe


def _inputs(c, drop):
    prob = case_problem(c)
    g = without_samples(prob['g'], drop)
    ks, bs, geom, hp = oracle_inputs(g)
    if not c.get('do_skip', True):
        hp = dict(hp, do_skip=False)
    return prob, g, ks, bs, geom, hp, t64(g['t_frames'])


def _reference(c, recipe, drop):
    prob, g, ks, bs, geom, hp, tf = _inputs(c, drop)
    tg = [t64(v) for v in case_targets(c, prob)]
    kind, out = reference_kind(c), {}
    if kind in ('f64', 't8'):
        loss, img, grads = ot.CpuTrainer(ks, bs, geom, hp).loss_and_grad(tf, tg[0], tg[1], tg[2], 1.0, c['dt'])
        out.update(loss=float(loss), images=img.detach().numpy(), grad=flat_grad(grads))
    if kind in ('emulator', 't8'):
        loss, img, grads = ob.Bf16Trainer(ks, bs, geom, hp, emulator_recipe(c, recipe)).loss_and_grad(tf, tg[0], tg[1], tg[2], 1.0, c['dt'])
        out.update(images=img.detach().numpy(), grad_emulator=ob.flat(grads))
        if kind == 'emulator':
            out.update(loss=float(loss), grad=out['grad_emulator'])
    out['cuts'] = tensor_cuts(g, c['depth'])
    return out


def _ties(c, recipe):
    _, g, ks, bs, geom, hp, tf = _inputs(c, None)
    em = None if reference_kind(c) == 'f64' else ob.Bf16Trainer(ks, bs, geom, hp, emulator_recipe(c, recipe))
    return tie_points(g, em, tf, c.get('do_skip', True))


def reference(name, c, recipe, drop=None):
    """dict(loss, images, grad (flat, flax tree order), cuts and, for the emulator kinds, grad_emulator) of the first step of a case
    (drop: without those ray samples), made once and read-only from then on."""
    return cached('step same bits', name, 'first step', recipe, drop, False, lambda: _reference(c, recipe, drop))


def reference_ties(name, c, recipe):
    """(H, W, G) bool: the ray samples with a ReLU tie on the forward of the case's own reference (the emulator's where it has one)."""
    return cached('step same bits', name, 'ties', recipe, None, False, lambda: _ties(c, recipe))


def bounds(c, recipe):
    """f32: images 1e-5 of their maximum, gradient GTOL / L2TOL['f32'] (x 2^(deg - 5) above degree 5, as
    gpu_support.check_general_path_problem); bf16 against the emulator: mlp_bounds' caps of the case's class (image, gradient L2, worst
    tensor L2); the 8-bit tape: the image cap against the emulator, GTOL / L2TOL['bf16'] against the float64 oracle."""
    deg, kind = c.get('deg', 3), reference_kind(c)
    k = max(1.0, 2.0 ** (deg - 5))
    if kind == 'f64':
        return dict(image=1e-5 * k, gmax=GTOL['f32'] * k, grad=L2TOL['f32'] * k)
    cls = 'fused128' if recipe == 'fused128' else problem_class(c['depth'], c.get('width', 256))
    caps = caps_of('random' if cls == 'deep' else cls, deg)
    if kind == 't8':
        return dict(image=caps['image'], gmax=GTOL['bf16'], grad=L2TOL['bf16'])
    return dict(caps)


def errors(first, ref):
    """The figures of a first step (same_bits.run_case's `first`) against its reference: image (max error / maximum), loss (relative),
    gmax (gradient max error / largest entry), grad (gradient relative L2), tensor (the worst relative L2 of one kernel / bias tensor)
    and, where the reference has one, grad_emulator."""
    img = first['images'].astype(np.float64).reshape(ref['images'].shape)
    gdev = first['grad'].astype(np.float64)
    assert np.abs(ref['images']).max() > 0 and np.abs(ref['grad']).max() > 0
    r = dict(image=maxerr(img, ref['images']), loss=abs(float(first['loss'].sum()) - ref['loss']) / abs(ref['loss']),
             gmax=maxerr(gdev, ref['grad']), grad=l2err(gdev, ref['grad']), tensor=max(tensor_l2(gdev, ref['grad'], ref['cuts'], True)))
    if 'grad_emulator' in ref:
        r['grad_emulator'] = l2err(gdev, ref['grad_emulator'])
    return r
