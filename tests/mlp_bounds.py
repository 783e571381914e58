"""The numbers and rules that more than one MLP kernel test reads: the tolerances against the float64 oracle, the figures observed
against the bf16 emulator and the bound rule built on them, the path the library takes for a network shape, the shape lists, the
mutant requirements, the error norms and the ReLU-tie adjudication of the case tables.  Plain numpy; no test here.  (The OBSERVED
tables of test_gpu_frame_chunks and test_gpu_buffer_contract stay in those files: nothing else reads them.)"""
import numpy as np

from oracle import oracle_bf16 as ob

# ---- against the float64 oracle (error / largest entry, and relative L2).  Set from what the kernels deliver on the golden fixtures
# (tools/debug/diag_tol.py): f32 mode 2e-5 for both (observed <= 1.6e-6), loss 1e-5 (observed <= 1.6e-6); bf16 mode L2 6e-2, max 1.2e-1,
# loss 3e-2 (observed <= 3.7e-2 / 7.5e-2 / 1.7e-2: bf16 activations and deltas on the tape, f32 accumulation, and only 100-500 points per
# fixture to average the rounding over -- the full-size test holds 2e-2)
GTOL = {'f32': 2e-5, 'bf16': 1.2e-1}       # max-norm
L2TOL = {'f32': 2e-5, 'bf16': 6e-2}        # relative L2
LOSSTOL = {'f32': 1e-5, 'bf16': 3e-2}
TOL = {'f32': 1e-5, 'bf16': 2e-2}          # emission (observed <= 9.4e-7 / 1.0e-2, tools/diag_tol.py)
IMG_TOL = {'f32': 1e-5, 'bf16': 1e-2}      # images (observed <= 6.8e-7 / 5.7e-3)


def l2err(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def maxerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def relerr(a, b):
    """maxerr of anything array-like, taken in float64; an all-zero reference gives inf or 0, not a division by zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def tensor_l2(grad, ref, cuts, skip_zero):
    """l2err of every kernel / bias tensor of a flat gradient (cuts: mlp_problems.tensor_cuts); skip_zero: 0 for a tensor whose
    reference is identically zero, which has no relative error."""
    return [0.0 if skip_zero and not np.linalg.norm(ref[c0:c1]) > 0 else l2err(grad[c0:c1], ref[c0:c1]) for c0, c1 in zip(cuts[:-1], cuts[1:])]


def tensor_label(i):
    """Tensor i of the flax order as the tests print it: K0, b0, K1, ..."""
    return ('K%d' if i % 2 == 0 else 'b%d') % (i // 2)


def first_difference(a, b):
    """None when the float32 arrays are bitwise equal, else (flat index, a, b) of the first element that differs."""
    d = np.nonzero(a.reshape(-1).view(np.uint32) != b.reshape(-1).view(np.uint32))[0]
    return None if d.size == 0 else (int(d[0]), float(a.reshape(-1)[d[0]]), float(b.reshape(-1)[d[0]]))


def held_or_adjudicated(label, first, within, ties, rerun, also=lambda second: True):
    """The ReLU-tie adjudication of a case table: (whether the case holds, the figures of its second run or None).  It holds when
    within(first); a miss is excused only if the reference's own forward has tied ray samples (ties(), called on a miss only) and
    the same case without exactly those samples (rerun(mask): Doppler weight 0 on both sides) meets the same bounds and the
    site's side conditions `also`.  No device access here: the site's callables do that."""
    if within(first):
        return True, None
    mask = ties()
    if not mask.any():
        return False, None
    second = rerun(mask)
    ok = bool(within(second) and also(second))
    print('relu ties (%s): %d tied ray samples taken out: %s' % (label, int(mask.sum()), 'adjudicated' if ok else 'NOT a tie'))
    return ok, second


# ---- the path of a network shape
def expected_recipe(depth, kernel_width, general):
    """The path the library's selection rules (common.h bhn_folds_wout, fused_bwd.hip ga0_chain_ok, bwd128_supported) give a bf16
    network -- written out here so that a change of the selection fails loudly instead of comparing against another recipe."""
    if general:
        return 'general'
    if kernel_width == 128 and depth == 4:
        return 'fused128'
    if depth < 3:
        return 'generic'
    return 'ga0_chain' if kernel_width == 256 else 'fold'


def kernel_width(w):
    return next(k for k in (32, 64, 128, 256) if w <= k) if w <= 256 else w


def problem_class(depth, width):
    """'deep': eight hidden layers at width >= 256 -- the bf16 rounding flips of the f32 accumulation compound down eight layers
    of the chain (not ties: taking the tied samples out does not move them), observed up to 3.1e-3 L2 / 1.4e-2 per tensor, the
    error growing from the output layer towards layer 0 (the per-layer profile check_case prints).  The emulator with float32
    instead of float64 accumulation (accum32) moves these problems by 1.6e-4 ... 5.8e-4 with the same profile, 10 ... 100x more
    than the shallow ones (tests/test_oracle_bf16_cpu.py::test_accumulation_noise_explains_the_largest_errors)."""
    return 'deep' if depth >= 8 and width >= 256 else 'random'


RANDOM_SHAPES = [(256, 4, 0, 3), (128, 4, 3, 3), (64, 8, 2, 3), (32, 6, 0, 3), (128, 4, 0, 0), (256, 4, 3, 1), (64, 4, 0, 2),
                 (128, 4, 2, 4), (100, 4, 0, 3), (48, 4, 3, 3), (200, 6, 0, 2), (20, 4, 0, 3), (64, 5, 0, 3), (128, 7, 2, 3),
                 (32, 3, 0, 3), (64, 2, 3, 2), (256, 5, 0, 3), (256, 8, 0, 3), (256, 8, 3, 3), (64, 4, 1, 3), (256, 6, 1, 2),
                 (256, 2, 0, 3)]           # test_random_problem_f32_and_bf16's 21 shapes + 2x256 (no W_out fold at the ga0_chain width)
GENERAL_SHAPES = [(128, 4, 3, 5), (512, 4, 0, 3), (300, 3, 1, 6), (64, 2, 0, 7), (384, 8, 2, 4), (512, 8, 0, 8), (40, 5, 3, 10)]
# Four Stokes planes (tests/stokes4_cases.py: what each shape is there for, with the LDS bytes of its tightest kernel at Sx = 4)
STOKES4_SHAPES = [(128, 4, 4, 3), (256, 4, 4, 3), (256, 8, 4, 3), (64, 6, 4, 3), (32, 3, 4, 3), (256, 2, 4, 3), (288, 4, 4, 3), (512, 4, 4, 6)]
# (depth, width) of the forms of the bf16 dW kernel's layer depth-1 job (fused_bwd.hip dw_kernel) that the shapes above leave out at a
# kernel width.  With do_skip the form follows from the depth: 3 = skip-concat into layer 2 and into the output layer, 4 = into layer
# 3, 5 = into the output layer only, 6 = neither.  RANDOM_SHAPES has depth 3 at width 32 only and no depth 5 (or 7) at width 32.
LAST_JOB_SHAPES = [(3, 64), (3, 128), (3, 256), (5, 32)]

# ---- bounds against the emulator (the f64 bounds of the same cases: 1e-2 images, 6e-2 / 3e-2 / 2e-2 gradient)
# Observed on the MI355X, per case (image error / maximum, emission relative L2, loss relative error, gradient relative L2 = the worst
# of the chi^2, recorded-tape and recompute routes, worst relative L2 of one kernel / bias tensor); for the cases with relu ties
# adjudicated (7x128, 8x256 S0, 8x384, 8x512) the figures of the problem without the tied samples.  The kernels are bitwise
# reproducible, so the bound of a case is 4x its own figure, capped at the required bound of its class (CAPS).
OBSERVED = {
    '4x256 S0 deg3':               (0.00017, 0.00018, 4e-07, 4.2e-05, 6.8e-05),
    '4x128 S3 deg3':               (0.00012, 0.0001, 1.4e-07, 2.5e-05, 4.2e-05),
    '8x64 S2 deg3':                (0.00012, 0.00012, 5.1e-07, 9.8e-05, 0.00026),
    '6x32 S0 deg3':                (1.4e-05, 3.4e-05, 1.4e-06, 1.7e-05, 3.8e-05),
    '4x128 S0 deg0':               (1.1e-05, 8.8e-06, 5.5e-08, 1.6e-06, 3.4e-06),
    '4x256 S3 deg1':               (0.00017, 0.00018, 1.6e-06, 0.0022, 0.0028),
    '4x64 S0 deg2':                (7e-05, 0.0001, 7.2e-08, 1.3e-05, 1.6e-05),
    '4x128 S2 deg4':               (0.00014, 7.2e-05, 1.6e-06, 4.2e-05, 0.00014),
    '4x100 S0 deg3':               (8.6e-05, 0.00018, 3.5e-07, 0.00055, 0.00099),
    '4x48 S3 deg3':                (6.1e-05, 0.00013, 4.1e-08, 2.6e-05, 4.7e-05),
    '6x200 S0 deg2':               (0.00015, 0.00023, 1.8e-06, 2.5e-05, 5.7e-05),
    '4x20 S0 deg3':                (1.2e-06, 1e-06, 2.8e-08, 5.8e-06, 2.3e-05),
    '5x64 S0 deg3':                (7e-05, 4.8e-05, 1.1e-06, 0.0002, 0.00053),
    '7x128 S2 deg3':               (9.9e-05, 0.00025, 1.1e-06, 0.00022, 0.00052),
    '3x32 S0 deg3':                (3e-05, 9.6e-05, 1.6e-07, 1.6e-05, 2.2e-05),
    '2x64 S3 deg2':                (2.4e-07, 4e-07, 5.9e-08, 2e-06, 6.7e-06),
    '5x256 S0 deg3':               (0.00017, 0.00016, 2.6e-06, 0.00025, 0.0007),
    '8x256 S0 deg3':               (0.00055, 0.00046, 2.1e-06, 0.00094, 0.0026),
    '8x256 S3 deg3':               (0.00034, 0.0005, 3.6e-07, 0.00082, 0.0027),
    '4x64 S1 deg3':                (3e-05, 1.8e-05, 1.7e-06, 3.5e-05, 8.7e-05),
    '6x256 S1 deg2':               (0.00014, 0.00024, 7.1e-06, 0.00012, 0.0003),
    '2x256 S0 deg3':               (4.5e-05, 4.8e-05, 6.8e-06, 2e-05, 6e-05),
    '4x128 S3 deg5':               (7.7e-05, 0.00014, 7.9e-08, 0.00044, 0.0014),
    '4x512 S0 deg3':               (9.6e-05, 0.00017, 2.8e-07, 4.6e-05, 0.00012),
    '3x300 S1 deg6':               (0.00013, 0.00017, 4.8e-06, 0.00022, 0.00066),
    '2x64 S0 deg7':                (0.00017, 0.00015, 7.5e-07, 3.5e-05, 5.7e-05),
    '8x384 S2 deg4':               (0.00042, 0.0004, 2.3e-06, 0.0016, 0.0055),
    '8x512 S0 deg8':               (0.00076, 0.00089, 1.3e-05, 0.0031, 0.014),
    '5x40 S3 deg10':               (0.00076, 0.00097, 9e-05, 0.00049, 0.0018),
    '3x64 S2 ragged':              (5.4e-05, 3.8e-05, 2.9e-06, 1.1e-05, 1.4e-05),
    '3x128 S2 ragged':             (2.1e-05, 6e-05, 3.2e-06, 1.2e-05, 9.2e-05),
    '3x256 S2 ragged':             (5.6e-05, 6.3e-05, 2.6e-06, 0.00036, 0.00067),
    '5x32 S2 ragged':              (3.8e-05, 5.7e-05, 6.3e-07, 0.00029, 0.0012),
    'g5_a full':                   (3.7e-07, 3.2e-07, 2.4e-07, 5.1e-08, 2.5e-07),
    'g5_a lc':                     (3.7e-07, 3.2e-07, 2.8e-07, 5.5e-08, 2.7e-07),
    'g5_b full':                   (3.9e-07, 3.7e-07, 1.1e-07, 1.1e-07, 2.8e-06),
    'g5_b lc':                     (3.9e-07, 3.7e-07, 2.5e-08, 1.1e-07, 2.8e-06),
    'g5_c full':                   (3.1e-07, 4.6e-07, 2.6e-08, 5.9e-08, 2e-07),
    'g5_c lc':                     (3.1e-07, 4.6e-07, 1.6e-07, 4.8e-08, 1.5e-07),
    'g5_d full':                   (1.6e-07, 2.8e-07, 2.2e-08, 4.7e-08, 5.3e-07),
    'g5_d lc':                     (1.6e-07, 2.8e-07, 1.4e-07, 4.7e-08, 5.3e-07),
    'g5_e full':                   (3.3e-07, 3.4e-07, 5.5e-09, 9.5e-07, 4.1e-06),
    'g5_e lc':                     (3.3e-07, 3.4e-07, 9.6e-09, 6.1e-07, 3.9e-06),
    'g5_f full':                   (2.4e-07, 2.8e-07, 1e-07, 3.6e-08, 2.7e-07),
    'g5_f lc':                     (2.4e-07, 2.8e-07, 8.7e-07, 3.7e-08, 5.8e-07),
    '4x128 rows 48 skip 1':        (0.00021, 0.00016, 4.8e-08, 2.2e-05, 6.2e-05),
    '4x128 rows 47 skip 1':        (0.00018, 0.00015, 3.8e-07, 2.8e-05, 8.9e-05),
    '4x128 rows 48 skip 0':        (8.2e-05, 7.1e-05, 3.9e-08, 2.5e-05, 7.9e-05),
    '4x128 rows 47 skip 0':        (8.6e-05, 7.4e-05, 3.5e-07, 2.3e-05, 7.6e-05),
    '4x113 rows 48 skip 1':        (0.00012, 9.6e-05, 2.7e-07, 3e-05, 7.6e-05),
    '4x113 rows 47 skip 1':        (0.00013, 0.00011, 1.7e-06, 3e-05, 9.5e-05),
    '4x113 rows 48 skip 0':        (0.00011, 0.00011, 3.7e-07, 2.7e-05, 9.1e-05),
    '4x113 rows 47 skip 0':        (0.00016, 0.0001, 2.3e-07, 3e-05, 0.00011),
    '4x97 rows 48 skip 1':         (0.00014, 8.9e-05, 1.2e-07, 1.7e-05, 7.1e-05),
    '4x97 rows 47 skip 1':         (8.8e-05, 9.4e-05, 7.9e-08, 1.5e-05, 4.7e-05),
    '4x97 rows 48 skip 0':         (0.00014, 0.00012, 1.6e-06, 3.5e-05, 0.0001),
    '4x97 rows 47 skip 0':         (0.0001, 0.00012, 2.2e-07, 2.6e-05, 7.3e-05),
    'config 2 subset masked':      (0.00018, 0.00014, 2.6e-07, 6.6e-05, 0.00013),
    'config 2 subset all_active':  (0.00015, 0.00015, 2.6e-06, 3.6e-05, 0.00011),
    'config 5 subset lc S3':       (0.00032, 0.00013, 5.7e-06, 5.6e-05, 0.00011),
    # four Stokes planes (tests/stokes4_cases.py, test_gpu_stokes4): image, gradient and worst tensor as every case prints them -- the
    # worst of its routes; emission and loss are not taken there (None)
    '4x128 S4 deg3':               (0.000128, None, None, 3.80e-05, 8.64e-05),
    '4x256 S4 deg3':               (0.000323, None, None, 4.43e-05, 7.83e-05),
    '8x256 S4 deg3':               (0.000248, None, None, 0.000125, 0.00034),
    '6x64 S4 deg3':                (0.000216, None, None, 7.82e-05, 0.000254),
    '3x32 S4 deg3':                (6.49e-07, None, None, 1.29e-07, 1.78e-07),
    '2x256 S4 deg3':               (6.36e-05, None, None, 1.50e-05, 4.95e-05),
    '4x288 S4 deg3':               (0.00019, None, None, 0.000478, 0.000923),
    '4x512 S4 deg6':               (0.00016, None, None, 0.00188, 0.00263),
    '4x128 S4 deg3 lc':            (0.000128, None, None, 6.15e-06, 1.27e-05),
    '4x128 S4 dense 96':           (0.000149, None, None, 7.97e-05, 0.000297),
    '4x128 S4 compacted':          (0.000123, None, None, 0.000121, 0.000245),
    '4x128 S4 span2':              (0.000302, None, None, 6.15e-05, 0.000139),
    '4x128 S4 x12':                (8.25e-05, None, None, 3.75e-05, 8.47e-05),
    '4x256 S4 ragged':             (0.00014, None, None, 7.27e-05, 0.000137),
    '8x256 S4 ragged':             (0.000334, None, None, 0.0012, 0.0026),
    '6x64 S4 ragged':              (9.03e-05, None, None, 2.96e-05, 4.27e-05),
    '4x288 S4 ragged':             (0.00016, None, None, 0.000105, 0.000286),
}
FIELDS = ('image', 'emission', 'loss', 'grad', 'tensor')
# required bounds (20x under the float64 comparisons' 1e-2 images / 6e-2 and 2e-2 gradient L2); 'deep' (8 hidden layers at width
# >= 256) is not capped: see problem_class
CAPS = {'golden': dict(image=5e-4, grad=3e-3, tensor=6e-3), 'random': dict(image=5e-4, grad=3e-3, tensor=6e-3),
        'fused128': dict(image=5e-4, grad=3e-3, tensor=6e-3), 'subset': dict(image=5e-4, grad=1e-3, tensor=2e-3), 'deep': dict()}


def caps_of(cls, deg=3):
    """CAPS[cls]; the image cap grows with the posenc degree above 5: octave i multiplies the f32 rounding of the warped coordinate by
    2^i before the sine, as in test_shapes_outside_the_fused_kernels."""
    return {k: cap * (max(1.0, 2.0 ** (deg - 5)) if k == 'image' else 1.0) for k, cap in CAPS[cls].items()}


def capped_bounds(fields, observed, caps):
    """The bound rule of every comparison with the emulator: per field 4x the observed figure (the kernels are bitwise reproducible),
    capped where `caps` names the field."""
    return {k: min(4.0 * v, caps.get(k, np.inf)) for k, v in zip(fields, observed)}


def bounds(name, cls, deg=3):
    """The bounds of test_gpu_bf16_faithful's case `name`: 4x OBSERVED, capped by CAPS[cls]."""
    return capped_bounds(FIELDS, OBSERVED[name], caps_of(cls, deg))


# Mutants (oracle_bf16.MUTANTS) that each case's bounds must see: distance >= 5x the bound in at least one bounded figure (gradient L2,
# one tensor, images).  Required: act_truncate on every case but TRUNC_BLIND; bias_scale on the goldens and on the fused 4x128 and
# config 2 / 5 cases (their per-tensor bounds see one output-bias entry x (1 + 2^-8)); drop_group on the goldens and the random /
# general-path problems but DROP_BLIND; dout_unrounded on the goldens.  Not required (distances printed, measured 0.1 ... 4x): dropping
# ONE 32-point group out of 2,000 ... 6,000 (fused 4x128, config 2 / 5) or leaving dout unrounded (3e-5 ... 1e-3 of the gradient)
# moves those problems by less than the kernels' accumulation noise does -- the float32-accumulating emulator (accum32) moves them
# by as much (tests/test_oracle_bf16_cpu.py::test_accumulation_noise_explains_the_largest_errors).
TRUNC_BLIND = {'8x512 S0 deg8'}          # 3x: eight layers at width 512, posenc degree 8 -- the noisiest problem (problem_class)
DROP_BLIND = {'4x100 S0 deg3', '5x256 S0 deg3', '5x40 S3 deg10', '8x256 S0 deg3', '8x384 S2 deg4', '8x512 S0 deg8'}


def mutant_ratios(variants, b, cuts):
    """{mutant: (gradient L2, worst tensor L2, image error / max, distance / bound)} from Bf16Trainer.loss_and_grad_variants."""
    _, i0, g0 = variants[None]
    g0, i0 = ob.flat(g0), i0.numpy()
    out = {}
    for m in ob.MUTANTS:
        _, i1, g1 = variants[m]
        g1 = ob.flat(g1)
        d = (l2err(g1, g0), max(tensor_l2(g1, g0, cuts, True)), maxerr(i1.numpy(), i0))
        out[m] = d + (max(d[0] / b['grad'], d[1] / b['tensor'], d[2] / b['image']),)
    return out


def required_mutants(name, cls):
    req = [] if name in TRUNC_BLIND else ['act_truncate']
    if cls in ('golden', 'fused128', 'subset'):
        req.append('bias_scale')
    if cls in ('golden', 'random', 'deep') and name not in DROP_BLIND:
        req.append('drop_group')
    return req + (['dout_unrounded'] if cls == 'golden' else [])


def check_mutants(name, cls, ratios):
    print('mutants %-26s %s' % (name, '  '.join('%s %.1e/%.1e/%.1e (%.1fx)' % ((m,) + v) for m, v in ratios.items())))
    for m in required_mutants(name, cls):
        assert ratios[m][3] >= 5.0, (name, m, ratios[m])
