"""Inputs and the float64 reference of the polarimetric EHT losses (libbhnerf_pol.so, observation.PolDFT), shared by
tests/test_pol_cpu.py and tests/test_gpu_pol.py.

Built on tests/eht_uv_cases.py: its blobs, dense128, FOV and MIN_AMP, and the generator of tests/closure_cases.py -- the same
draws in the same order (stations, images, a second draw of images for the data, the visibility sigmas, the closure-phase sigmas,
the log-closure-amplitude sigmas); sigma_pvis and sigma_m, uniform(0.05, 0.2) times the mean |target| of their term, are drawn
last.  The data are the float64 P = Q + iU and m = P / I of the second draw: one complex target and one sigma per frame and
baseline.

The reference is float64 torch autograd of  scale * sum_d w_d chi^2_d  on a dense complex128 A, as closure_cases.closure_loss is.
m has a pole at I = 0: every case has min |I| / max |I| >= MIN_AMP on plane 0 of the images the loss is taken at, asserted in
case()."""
import numpy as np
import torch

import closure_cases as K
import eht_uv_cases as E
from bhnerf_amd import observation

TERMS = observation.POL_TERMS
DTYPES = ('pvis', 'm', 'pvis+m')
# name -> (H, W, B, seed, stations).  '13x7': nvis 6, fewer than a baseline block of 8.  '12x20': B = 3, nvis 10, two baseline
# blocks.  '9x11': nvis 45.  '8x8': 24 stations, nvis 276 -- more baselines than the 256 lanes of a workgroup, so the lanes wrap.
CASES = {'13x7': K.CASES['13x7'], '12x20': K.CASES['12x20'], '9x11': K.CASES['9x11'], '8x8': (8, 8, 1, 10, 24)}
PARAMS = [(name, Sx) for name in CASES for Sx in (3, 4)]
WEIGHTS = {'pvis': 0.5, 'm': 0.25}                    # the non-unit weights of the parity tests
SCALE = 2.0
MUTANTS = ('P = Q - iU', 'no d/dI', 'conj target', 'plane 3 <- plane 2')

# Largest error of the 'm' term against float64 over PARAMS and the dtypes that hold 'm', weights WEIGHTS, scale SCALE, measured
# on an MI355X (tests/test_gpu_pol.py prints every figure).  'loss': the term and the totals that hold it, relative (largest: the
# 'pvis+m' total at 13x7, Sx 4, 1.3e-7; the term itself 8.6e-8); 'dimages': relative to the largest element (largest: 'pvis+m' at
# 8x8, Sx 4, 3.8e-7).  Bounded at ten times the measurement and never above 1e-3 -- the rule of DESIGN 4.15 for 'logcamp': the
# margin covers float32 division near the 1 / I pole on other inputs.  The host build (tests/test_pol_cpu.py, g++ -O2
# -ffp-contract=off) gives 3.3e-7 and 5.0e-7 on the same cases.  'pvis' is linear like 'vis' and takes the project's 2e-5 (measured
# 1.2e-7 / 3.1e-7).
MEASURED_M = {'loss': 1.3e-7, 'dimages': 3.8e-7}
M_BOUND = {k: min(10.0 * v, 1e-3) for k, v in MEASURED_M.items()}


def bound(names, what):
    """The bound of a figure made of the terms `names`; what: 'loss' or 'dimages'."""
    return M_BOUND[what] if 'm' in names else E.F32_TOL


def pol_loss(images, A, data, terms, weights, scale, mutant=None):
    """float64: (total, d total / d images, {term: scale w_d chi^2_d}, visibilities) of scale * sum_d w_d chi^2_d.
    images (B, Sx, H, W); A (B, nvis, R) complex128; data {term: (target complex (B, nvis), sigma (B, nvis))}.  `mutant`: one of
    MUTANTS, a deliberately wrong variant that the tests must tell from the reference."""
    img = torch.tensor(np.asarray(images, dtype=np.float64), requires_grad=True)
    At = torch.tensor(A)
    B, Sx = img.shape[:2]
    vec = img.reshape(B, Sx, -1).to(torch.complex128)
    vis = torch.einsum('bkr,bsr->bsk', At, vec)
    P = vis[:, 1] + (-1j if mutant == 'P = Q - iU' else 1j) * vis[:, 2]
    V0 = vis[:, 0].detach() if mutant == 'no d/dI' else vis[:, 0]
    parts = {}
    for d in terms:
        tg = torch.tensor(np.asarray(data[d][0], dtype=np.complex128))
        sg = torch.tensor(np.asarray(data[d][1], dtype=np.float64))
        if mutant == 'conj target':
            tg = tg.conj()
        q = P if d == 'pvis' else P / V0
        parts[d] = scale * weights[d] * (((q - tg).abs() / sg) ** 2).sum()
    total = sum(parts[d] for d in terms)
    total.backward()
    grad = img.grad.numpy().copy()
    if mutant == 'plane 3 <- plane 2' and Sx == 4:
        grad[:, 3] = grad[:, 2]
    return total.item(), grad, {d: v.item() for d, v in parts.items()}, vis.detach().numpy()


_CASES, _REFS = {}, {}


def case(name, Sx, spec=None):
    """Everything about one input set, computed once and left unchanged: uv, pairs, images (B, Sx, H, W) float32, data {term:
    (target complex64 (B, nvis), sigma float32 (B, nvis))}, the dense A and the float64 visibilities of the images.
    spec: an explicit (H, W, B, seed, stations) under a name of the caller's instead of a row of CASES (tests/eht_edge_cases.py)."""
    key = (name, Sx) if spec is None else (name, Sx, tuple(spec))
    if key in _CASES:
        return _CASES[key]
    H, W, B, seed, ns = spec if spec is not None else CASES[name]
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(B, ns, 2)) * 3e9
    pairs = np.array([(i, j) for i in range(ns) for j in range(i + 1, ns)])
    uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])
    shape = (B, Sx, H, W)
    images, truth = E.blobs(rng, shape), E.blobs(rng, shape)
    A = E.dense128(uv, E.FOV, H, W)
    vis_of = lambda im: np.einsum('bkr,bsr->bsk', A, im.astype(np.float64).reshape(B, Sx, H * W))
    vis_truth, vis = vis_of(truth), vis_of(images)
    # the draws of closure_cases.case, in its order: visibility sigmas, one per closure phase (every station triple), one per log
    # closure amplitude (two per station quadruple)
    ncp, nca = ns * (ns - 1) * (ns - 2) // 6, 2 * (ns * (ns - 1) * (ns - 2) * (ns - 3) // 24)
    rng.uniform(0.5, 1.5, vis_truth.shape)
    rng.uniform(0.05, 0.2, (B, Sx, ncp))
    rng.uniform(0.05, 0.2, (B, Sx, nca))
    op = observation.PolDFT(uv, E.FOV, (H, W))
    data = {}
    for t, target in (('pvis', op.polarised_visibility(vis_truth)), ('m', op.fractional_polarisation(vis_truth))):
        sigma = rng.uniform(0.05, 0.2, target.shape) * np.abs(target).mean()
        data[t] = (target.astype(np.complex64), sigma.astype(np.float32))
    amp = np.abs(vis[:, 0])
    out = dict(name=name, H=H, W=W, B=B, ns=ns, Sx=Sx, uv=uv, pairs=pairs, images=images, data=data, A128=A, vis=vis,
               min_amp=float(amp.min() / amp.max()), max_m=float(np.abs(op.fractional_polarisation(vis)).max()))
    assert out['min_amp'] >= E.MIN_AMP, (name, Sx, out['min_amp'])                     # off the 1 / I pole
    _CASES[key] = out
    return out


def reference(c, dtype, weights=None, scale=1.0, mutant=None):
    """(total, grad, {term: value}, vis) of the float64 reference for one '+'-joined dtype, computed once per argument set."""
    weights = dict({t: 1.0 for t in TERMS}, **(weights or {}))
    key = (c['name'], c['Sx'], dtype, tuple(sorted(weights.items())), scale, mutant)
    if key not in _REFS:
        _REFS[key] = pol_loss(c['images'], c['A128'], c['data'], dtype.split('+'), weights, scale, mutant)
    return _REFS[key]


def operator(c, weights=None):
    """The PolDFT of a case."""
    return observation.PolDFT(c['uv'], E.FOV, (c['H'], c['W']), weights=weights)


def packed(c, dtype):
    """(target, sigma) of `dtype`: the terms' arrays concatenated along the last axis in the canonical order."""
    terms = dtype.split('+')
    return (np.concatenate([c['data'][t][0] for t in terms], axis=-1), np.concatenate([c['data'][t][1] for t in terms], axis=-1))


def errors(dtype, total, parts, grad, ref):
    """Relative errors against reference(): {'total', 'pvis', 'm' (present terms), 'dimages' (when grad is given)}."""
    ref_total, ref_grad, ref_parts, _ = ref
    out = {'total': abs(total - ref_total) / abs(ref_total)}
    for t in dtype.split('+'):
        out[t] = abs(parts[t] - ref_parts[t]) / abs(ref_parts[t])
    if grad is not None:
        out['dimages'] = E.rel_max(grad, ref_grad)
    return out
