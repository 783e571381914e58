"""The cases and the float64 reference of the volume priors (libbhnerf_reg.so, include/bhnerf_reg.h), shared by
tests/test_vol_reg_cpu.py (the CPU build of the plan) and tests/test_gpu_vol_reg.py (the kernels).  Imported by the tests the way
gr_factor_cases.py is.

The reference is torch autograd in float64 on the formulas of the header, written with whole-array slices: it shares no code and
no loop structure with csrc/vol_reg.h.

The kernel's plan (csrc/vol_reg.h): a workgroup of 256 lanes takes a chunk of 1024 voxels, a lane 4 voxels 256 apart.  A lane
takes a second trip from 257 voxels on (13x7x11 = 1001 voxels and every larger case); a volume has a second workgroup from 1025
voxels on (33x17x9 = 5049: 5 workgroups); the sum kernel's lanes take a second trip over the workgroups' partial sums from 257
workgroups on, i.e. above 262144 voxels: 64x64x64 is exactly 256 workgroups, so 'second_sum_trip' (66x64x64, 264 workgroups) is
the case that takes it."""
import numpy as np
import torch

SEED = 7
SPACING = (0.5, 0.25, 0.125)
WEIGHTS = (1.0, 0.3, 0.2)
EPS = 1e-3
SCALE = 0.7
TERMS = ('tv', 'tsv', 'l1')
SINGLE_WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))

# name -> (dims, N, frac); frac None: mask = None
RANDOM_CASES = {
    '1x1x1': ((1, 1, 1), 1, 1.0),
    '2x1x1': ((2, 1, 1), 1, 1.0),
    '1x1x5': ((1, 1, 5), 2, 1.0),
    '5x7x3': ((5, 7, 3), 1, 0.7),
    '13x7x11': ((13, 7, 11), 3, 0.7),
    '33x17x9': ((33, 17, 9), 2, 0.6),
    '64x64x64': ((64, 64, 64), 1, 0.5),
    'second_sum_trip': ((66, 64, 64), 1, 0.5),
    'no_mask': ((13, 7, 11), 2, None),
}
MUTANT_CASES = ('5x7x3', '13x7x11', '33x17x9')
BIG_CASES = ('64x64x64', 'second_sum_trip')


def make_case(name):
    """dict(e (N, nx, ny, nz) float32, mask (nx, ny, nz) uint8 or None, spacing, weights, eps, scale) of a named case."""
    if name in RANDOM_CASES:
        dims, N, frac = RANDOM_CASES[name]
        rng = np.random.default_rng(SEED)
        e = rng.uniform(0.0, 1.0, (N,) + dims).astype(np.float32)
        mask = None
        if frac is not None:
            mask = (rng.uniform(0.0, 1.0, dims) < frac).astype(np.uint8)
            e = e * mask
        return dict(e=e, mask=mask, spacing=SPACING, weights=WEIGHTS, eps=EPS, scale=SCALE)
    if name in ('all_zero_mask', 'single_voxel_mask'):
        base = make_case('no_mask')
        mask = np.zeros(base['e'].shape[1:], dtype=np.uint8)
        if name == 'single_voxel_mask':
            mask[4, 3, 5] = 1
        return dict(base, mask=mask)
    if name in ('smooth_eps1e-6', 'smooth_eps1e-3'):
        return smooth_case(1e-6 if name.endswith('1e-6') else 1e-3)
    raise KeyError(name)


def smooth_case(eps):
    """24x20x16: a Gaussian hotspot of sigma 1.5 M at (5.5, 0, 0) on a 4.5e-5 floor over +-10, +-10, +-4 M, with the domain mask
    3 <= r <= 10, |z| <= 3: the emission a recovery produces, at the spacing of its lattice."""
    dims, half = (24, 20, 16), (10.0, 10.0, 4.0)
    axes = [np.linspace(-h, h, n) for h, n in zip(half, dims)]
    x, y, z = np.meshgrid(*axes, indexing='ij')
    r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    mask = ((r >= 3.0) & (r <= 10.0) & (np.abs(z) <= 3.0)).astype(np.uint8)
    e = 4.5e-5 + np.exp(-((x - 5.5) ** 2 + y ** 2 + z ** 2) / (2 * 1.5 ** 2))
    e = (e * mask).astype(np.float32)[None]
    spacing = tuple(float(a[1] - a[0]) for a in axes)
    return dict(e=e, mask=mask, spacing=spacing, weights=WEIGHTS, eps=eps, scale=SCALE)


ALL_CASES = tuple(RANDOM_CASES) + ('all_zero_mask', 'single_voxel_mask', 'smooth_eps1e-6', 'smooth_eps1e-3')


def reference(e, mask, spacing, weights, eps, scale, want_grad=True, mutant=None):
    """float64: (loss[4] = total, tv, tsv, l1 each scale w_d term_d; per_volume (3, N) unscaled; grad (N, nx, ny, nz) or None).
    `mutant` names one of the wrong variants of MUTANTS."""
    e64 = torch.tensor(np.asarray(e, dtype=np.float64), requires_grad=want_grad)
    m = torch.ones(e64.shape[1:], dtype=torch.float64) if mask is None else torch.tensor(np.asarray(mask, dtype=np.float64))
    h = list(spacing)
    if mutant == 'strides_swapped':              # the volume read with the x and z strides swapped
        src = e64.reshape(e64.shape[0], -1)
        nx, ny, nz = e64.shape[1:]
        idx = (np.arange(nx)[:, None, None] * 1 + np.arange(ny)[None, :, None] * nz + np.arange(nz)[None, None, :] * (ny * nz))
        idx = np.minimum(idx, nx * ny * nz - 1)
        vol = src[:, torch.tensor(idx.reshape(-1))].reshape(e64.shape)
    else:
        vol = e64
    d = []
    for axis in range(3):
        n = vol.shape[1 + axis]
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[1 + axis], hi[1 + axis] = slice(0, n - 1), slice(1, n)
        both = m[tuple(lo[1:])] * (torch.ones_like(m[tuple(hi[1:])]) if mutant == 'neighbour_mask_ignored' else m[tuple(hi[1:])])
        diff = (vol[tuple(hi)] - vol[tuple(lo)]) * both
        if mutant != 'no_inverse_h':
            diff = diff / h[axis]
        full = torch.zeros_like(vol)
        if mutant == 'stored_at_v_plus_1':
            full[tuple(hi)] = diff
        else:
            full[tuple(lo)] = diff
        d.append(full)
    q = d[0] ** 2 + d[1] ** 2 + d[2] ** 2
    eps2 = eps if mutant == 'eps_not_squared' else eps * eps
    zero = torch.zeros(e64.shape[0], dtype=torch.float64)
    tv = (m * torch.sqrt(q + eps2)).sum(dim=(1, 2, 3)) if weights[0] != 0 else zero
    tsv = (m * q).sum(dim=(1, 2, 3)) if weights[1] != 0 else zero
    l1 = (m * vol.abs()).sum(dim=(1, 2, 3)) if weights[2] != 0 else zero
    per_volume = torch.stack([tv, tsv, l1])
    terms = torch.stack([scale * w * t.sum() for w, t in zip(weights, (tv, tsv, l1))])
    total = terms.sum()
    grad = None
    if want_grad:
        if total.requires_grad:
            total.backward()
        grad = (e64.grad if e64.grad is not None else torch.zeros_like(e64)).numpy().copy()
    loss = np.concatenate([[float(total.detach())], terms.detach().numpy()])
    return loss, per_volume.detach().numpy(), grad


MUTANTS = ('stored_at_v_plus_1', 'neighbour_mask_ignored', 'no_inverse_h', 'eps_not_squared', 'strides_swapped')


def grad_error(got, ref):
    """max |got - ref| relative to the largest element of ref (absolute when ref is all zero)."""
    top = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()) / (top if top > 0 else 1.0)


def loss_error(got, ref):
    """|got - ref| / |ref| per slot (absolute where ref is 0), the largest."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.where(ref != 0, np.abs(ref), 1.0)
    return float((np.abs(got - ref) / den).max())
