"""What the GPU tests of the MLP and stand-alone kernels share and that needs a device: the `dev` and `lib` fixtures (a test module
imports them by name), raw buffers for calls through the C ABI (ptr, stream_ptr, place, Out), the one device setup of a problem, the
one check of the path that ran (assert_path: pure Python on engine.tape_info, held to its rules by test_mlp_harness_cpu), and
the random-problem checks that test_gpu_backward and the fuzzers under tools/ run.  No test here."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_tree
from mlp_bounds import GTOL, L2TOL, l2err
from mlp_problems import RANDOM_PROBLEM_DOMAIN, RANDOM_PROBLEM_JITTER, RANDOM_PROBLEM_SHAPE, f32, random_problem, without_samples
from oracle import oracle_bf16 as ob
from oracle import oracle_np as onp


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from bhnerf_amd import _hip
    return _hip.lib()


# ---- raw buffers for calls through the C ABI
def stream_ptr(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def place(arr, dev, shift=0):
    """`arr` on the device as a contiguous view that starts `shift` elements into a fresh allocation: shift 1 is a 4-byte
    aligned float view, shift 2 an 8-byte aligned one.  complex64 goes as pairs of floats."""
    a = np.ascontiguousarray(arr)
    if a.dtype == np.complex64:
        a = a.view(np.float32)
    buf = torch.zeros(a.size + shift + 8, dtype=torch.from_numpy(a.reshape(-1)[:1]).dtype, device=dev)
    assert buf.data_ptr() % 256 == 0
    view = buf[shift:shift + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.is_contiguous() and view.data_ptr() % 16 == (shift * a.itemsize) % 16
    return view


class Out:
    """An output of n elements inside a buffer filled with `sentinel` (uint8: 0xA5): `guard` elements before, `guard` after."""

    def __init__(self, n, dev, shift=0, dtype=torch.float32, init=None, *, guard, sentinel):
        self.n, self.lo = int(n), guard + shift
        self.fill = 0xA5 if dtype == torch.uint8 else sentinel
        self.buf = torch.full((self.lo + self.n + guard,), self.fill, dtype=dtype, device=dev)
        self.view = self.buf[self.lo:self.lo + self.n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))
        assert self.view.data_ptr() % 16 == (shift * self.buf.element_size()) % 16

    def numpy(self):
        before, after = self.buf[:self.lo], self.buf[self.lo + self.n:]
        assert bool((before == self.fill).all()) and bool((after == self.fill).all()), 'a store landed outside the output'
        return self.view.cpu().numpy().copy()

    def untouched(self):
        return bool((self.buf == self.fill).all())


# ---- the device side of a problem
def ray_args(g):
    """The ray-tracing arguments of a g5-layout problem as the reference-shaped API takes them: float32 arrays, J = 1.0 for none."""
    rt = {k: f32(g[k]) for k in ('coords', 'Omega', 'g', 'dtau', 'Sigma', 't_geos')}
    return dict(rt, J=(f32(g['J']) if np.ndim(g['J']) else 1.0), t_start_obs=float(g['t_start_obs']), t_injection=float(g['t_injection']))


def predictor_of(g, mode, dev, do_skip=None):
    from bhnerf_amd import network
    hp = g['hparams']
    kw = {} if do_skip is None else dict(do_skip=do_skip)
    return network.NeRF_Predictor(hp[0], hp[1], hp[2], hp[3], posenc_deg=int(hp[4]), net_depth=int(hp[5]), net_width=int(hp[6]), mode=mode,
                                  device=dev, **kw)


def device_setup(g, mode, dev, drop=None, do_skip=None):
    """The device side of a g5-layout problem, in this order: NeRF_Predictor -> engine() -> geometry(...) -> flatten -> frame_offsets.
    Returns (predictor, engine, geometry, flat parameters, tM0); nothing is packed, and a workspace cap is the caller's to set on the
    engine.  drop: the tie adjudication's ray samples (Doppler weight 0)."""
    from bhnerf_amd import engine as E
    g = without_samples(g, drop)
    rt = ray_args(g)
    pred = predictor_of(g, mode, dev, do_skip)
    eng = pred.engine()
    geom = pred.geometry(rt['coords'], rt['Omega'], rt['t_geos'], rt['J'] if np.ndim(g['J']) else None, rt['g'], rt['dtau'], rt['Sigma'])
    flat = eng.flatten(golden_tree(g))
    tM0 = E.frame_offsets(g['t_frames'], rt['t_start_obs'], rt['t_injection'], onp.GM_C3_SGRA_HR, dev)
    return pred, eng, geom, flat, tM0


def expected_flags(recipe):
    """The engine.tape_info flags of a path: a recipe of oracle_bf16, 't8' (the 8-bit tape: the fold, dW_0 left in the dW kernel),
    'f32', or 'general' / 'general f32'."""
    return dict(general=recipe.startswith('general'), fused128=recipe == 'fused128', ga0_chain=recipe == 'ga0_chain',
                drop_ga=recipe in ('fold', 'ga0_chain', 't8'))


def assert_path(name, eng, geom, mode, recipe, general, compact=None, tile_groups=None):
    """The path that runs is the one the case `name` is listed (and, in the bf16 modes, emulated) for -> (flags, info) of
    engine.tape_info.  mode 'f32', 'bf16' or 'bf16_t8'; recipe: expected_flags' (ignored in f32; the emulator has no recipe of its own
    for 't8', which folds W_out as 'fold' does); compact: whether the layout is point-compacted; tile_groups: the 32-point groups per
    tile of the training forward."""
    info = eng.tape_info((geom.P_eff + 31) // 32)
    flags = info['flags']
    assert flags['general'] == general, (name, flags)
    if mode == 'f32':
        assert not (flags['fused128'] or flags['ga0_chain'] or flags['drop_ga']), (name, flags)
    else:
        want = expected_flags(recipe)
        assert want['general'] == general and ob.recipe_for(flags) == ('fold' if recipe == 't8' else recipe), (name, flags, recipe)
        assert flags['fused128'] == want['fused128'] and flags['ga0_chain'] == want['ga0_chain'], (name, flags, recipe)
        assert general or flags['drop_ga'] == want['drop_ga'], (name, flags, recipe)      # (fused128: the fold is bwd128_kernel's own)
    if compact is not None:
        assert (geom.compact is not None) == compact, (name, 'layout')
    if tile_groups is not None:
        assert info['fwd_groups_per_tile'] == tile_groups, (name, info)
    return flags, info


def chi2_step(pred, flat, rt, t_frames, target, sigma, offset, scale=1.0, dt='full'):
    """network.loss_fn_image on the flat parameters `flat` through the reference-shaped API (rt: the ray-tracing arguments, as ray_args
    gives them) and its backward -> (loss, images, the float32 gradient as a numpy array)."""
    from bhnerf_amd import network, units
    params = flat.requires_grad_(True)
    tree = network.ParamTree(); tree.flat = params
    loss, [images] = network.loss_fn_image(tree, pred.apply, target, sigma, offset, t_frames, rt['coords'], rt['Omega'], rt['J'], rt['g'],
                                           rt['dtau'], rt['Sigma'], rt['t_start_obs'], rt['t_geos'], rt['t_injection'], scale, units.hr, dt)
    loss.backward()
    return loss, images.detach(), params.grad.cpu().numpy()


def problem_of(tree, geo, t_frames, t_injection, dom, deg, depth, width):
    """A tree + geometry dict (J: an array or None) + recovery domain in g5 layout, for device_setup / mlp_problems.oracle_inputs."""
    g = {k: geo[k] for k in ('coords', 'Omega', 't_geos', 'g', 'dtau', 'Sigma')}
    g.update(J=np.array(1.0) if geo.get('J') is None else geo['J'], t_frames=t_frames, t_start_obs=0.0, t_injection=t_injection,
             hparams=np.array(list(dom) + [deg, depth, width, 1.0]))
    for i in range(depth + 1):
        g['kernel%d' % i], g['bias%d' % i] = tree['MLP_0']['Dense_%d' % i]['kernel'], tree['MLP_0']['Dense_%d' % i]['bias']
    return g


# ---- random problems against the float64 oracle (test_gpu_backward; tools/fuzz_parity.py and tools/fuzz_tape8.py with their draws)
def random_problem_errors(prob, mode, dev, grad_out=None):
    """(image error / image maximum, gradient max error / largest entry, gradient relative L2) of the HIP path against the
    float64 oracle on a random_problem(); `grad_out` (a list) receives the device gradient."""
    g, S, img_ref, gref = prob['g'], prob['S'], prob['img_ref'], prob['gref']
    pred = predictor_of(g, mode, dev)
    # one Stokes plane: the reference squeezes the unit axis (network.py:418), so its images -- and the targets a caller
    # pairs them with -- are (B, H, W); the oracle trainer keeps the axis
    sq = (lambda v: v[:, 0]) if S == 1 else (lambda v: v)
    _, images, gdev = chi2_step(pred, pred.engine().flatten(golden_tree(g)), ray_args(g), prob['t_frames'], sq(prob['target']), sq(prob['sigma']),
                                sq(prob['offset']))
    img = images.cpu().numpy().reshape(img_ref.shape)
    if float(img_ref.abs().max()) == 0.0 or float(np.abs(gref).max()) == 0.0:
        # an empty recovery domain (the fuzz draws thin shells no sample falls into): the reference image and gradient are
        # identically zero, and so must the device's be -- there is no scale to take an error relative to
        assert float(img_ref.abs().max()) == 0.0 and float(np.abs(gref).max()) == 0.0
        assert not img.any() and not gdev.any(), (mode, 'non-zero output for an empty domain')
        return 0.0, 0.0, 0.0
    ierr = np.abs(img - img_ref.numpy()).max() / img_ref.abs().max().item()
    if grad_out is not None:
        grad_out.append(gdev)
    return ierr, np.abs(gdev - gref).max() / np.abs(gref).max(), l2err(gdev, gref)


def adjudicate_relu_ties(width, depth, S, deg, dev, gerr, ties, **where):
    """A detected ReLU tie is only an explanation if the SAME problem without the tied ray samples meets the f32 bounds:
    those samples get Doppler weight g = 0 on both sides (no contribution to the image, hence none to the gradient), every
    other sample keeps its inputs and its forward values.  Anything else is reported as a failure of the original."""
    prob = random_problem(width, depth, S, deg, drop_ties=True, **where)
    assert prob['ties_left'] == 0 and 0 < prob['dropped'] <= ties
    ierr, g2, l2 = random_problem_errors(prob, 'f32', dev)
    assert ierr < 1e-5 and g2 < GTOL['f32'] and l2 < L2TOL['f32'], ('f32', gerr, ties, 'NOT a tie: without the %d tied samples %g / %g' % (prob['dropped'], g2, l2))
    print('relu ties adjudicated: %d ties on %d ray samples, gradient error %.2e; without those samples: error %.2e (L2 %.2e)'
          % (ties, prob['dropped'], gerr, g2, l2))


def check_random_problem(dev, width, depth, S, deg, shape=RANDOM_PROBLEM_SHAPE, domain=RANDOM_PROBLEM_DOMAIN, jitter=RANDOM_PROBLEM_JITTER):
    """The body of test_random_problem_f32_and_bf16: a random_problem on the fused kernels, both modes, against the float64 oracle."""
    where = dict(shape=shape, domain=domain, jitter=jitter)
    prob = random_problem(width, depth, S, deg, **where)
    for mode in ('f32', 'bf16'):
        ierr, gerr, l2 = random_problem_errors(prob, mode, dev)
        tol_img = {'f32': 1e-5, 'bf16': 1e-2}[mode]
        assert ierr < tol_img, (mode, ierr)
        ties = prob['ties']
        if mode == 'f32' and ties and not (gerr < GTOL[mode] and l2 < L2TOL[mode]):
            adjudicate_relu_ties(width, depth, S, deg, dev, gerr, ties, **where)        # raises unless the ties explain it
            continue
        assert gerr < GTOL[mode], (mode, gerr, ties)
        assert l2 < L2TOL[mode], (mode, l2, ties)


def check_general_path_problem(dev, width, depth, S, deg, shape=RANDOM_PROBLEM_SHAPE, domain=RANDOM_PROBLEM_DOMAIN, jitter=RANDOM_PROBLEM_JITTER):
    """The body of test_shapes_outside_the_fused_kernels: a random_problem on the general path, both modes, bitwise reproducible."""
    where = dict(shape=shape, domain=domain, jitter=jitter)
    prob = random_problem(width, depth, S, deg, **where)
    tol_f32 = 1e-5 * max(1.0, 2.0 ** (deg - 5))
    for mode in ('f32', 'bf16'):
        out = []
        ierr, gerr, l2 = random_problem_errors(prob, mode, dev, grad_out=out)
        print('general path %dx%d deg %d S %d %s: image %.2e  gradient max %.2e  L2 %.2e  ties %d' % (depth, width, deg, S, mode, ierr, gerr, l2, prob['ties']))
        again = []
        random_problem_errors(prob, mode, dev, grad_out=again)
        assert np.array_equal(out[0], again[0]), (mode, 'not reproducible', np.abs(out[0] - again[0]).max())
        if mode == 'bf16':
            assert ierr < 1e-2, (mode, ierr)
            assert gerr < GTOL['bf16'], (mode, gerr, prob['ties'])
            assert l2 < L2TOL['bf16'], (mode, l2, prob['ties'])
            continue
        assert ierr < tol_f32, (mode, ierr)
        if prob['ties'] and not (gerr < GTOL['f32'] * tol_f32 / 1e-5 and l2 < L2TOL['f32'] * tol_f32 / 1e-5):
            adjudicate_relu_ties(width, depth, S, deg, dev, gerr, prob['ties'], **where)
            continue
        assert gerr < GTOL['f32'] * tol_f32 / 1e-5 and l2 < L2TOL['f32'] * tol_f32 / 1e-5, (mode, gerr, l2)
