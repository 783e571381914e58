"""Inputs and the float64 reference of the matrix-free EHT losses (libbhnerf_eht.so, observation.DirectDFT), shared by
tests/test_eht_uv_cpu.py and tests/test_gpu_eht_uv.py.

The reference is the TABLE form in float64: a dense complex128 A (B, nvis, H W) from the formula of observation.dft_matrix, the
visibilities A . image, and for closure phases the bispectrum through (tri, tri_sign) -- each baseline's visibility once, a
conjugate where the sign is -1.  Loss and image gradient come from torch's complex autograd.  tests/test_eht_uv_cpu.py holds it
to oracle_np.loss_eht and to dense_ref_loss below (the dense conjugated-legs form of tests/test_gpu_eht.py) at the small shapes.

Inputs: station positions rng.normal(size=(B, ns, 2)) * 3e9 wavelengths, every station pair a baseline, every triple a triangle;
field of view 16 M of Sgr A*; images a Gaussian blob plus 5 % uniform noise, normalised to ~2 Jy.  The data (target) are the
visibilities of a second draw of such images, so that the residuals are of the size of the signal."""
import numpy as np
import torch

from bhnerf_amd import observation

RAD_PER_M = 5.03e-6 / 3600.0 * np.pi / 180.0          # GM/c^2/D of Sgr A* in radians, as in tests/test_gpu_eht2017.py
FOV = 16.0 * RAD_PER_M
F32_TOL = 2e-5                                        # the project's f32 bound
MIN_AMP = 0.05                                        # smallest |vis| / largest |vis| a 'cphase' case may have (1 / |vis| pole)

# name -> (H, W, B, seed, stations)
CASES = {'12x20': (12, 20, 3, 0, 5), '13x7': (13, 7, 2, 1, 4)}
BIG = (64, 64, 2, 5, 20)                              # 190 baselines, 1140 triangles: the seed satisfies MIN_AMP (asserted)


def dense_ref_loss(images, A, target, sigma, scale, dtype):
    """(loss, d loss / d images) of the dense-matrix EHT chi^2 by float64 complex autograd; 'cphase': A holds the three conjugated legs."""
    img = torch.tensor(images, dtype=torch.float64, requires_grad=True)
    At, tg, sg = torch.tensor(A), torch.tensor(target), torch.tensor(sigma)
    vec = img.reshape(img.shape[0], -1, 1).to(torch.complex128)
    if dtype == 'cphase':
        vis = (At.to(torch.complex128) @ vec[:, None]).squeeze(-1)
        loss = scale * ((1.0 - torch.cos(tg - torch.angle(vis.prod(dim=-2)))) / sg ** 2).sum()
    else:
        vis = (At.to(torch.complex128) @ vec).squeeze(-1)
        loss = scale * (((vis - tg).abs() / sg) ** 2).sum() if dtype == 'vis' else scale * (((vis.abs() - tg) / sg).abs() ** 2).sum()
    loss.backward()
    return loss.item(), img.grad.numpy()


def blobs(rng, shape):
    """(..., H, W) float32: a Gaussian blob plus 5 % uniform noise per plane, ~2 Jy in total."""
    H, W = shape[-2:]
    yy, xx = np.meshgrid(np.arange(H) - (H - 1) / 2.0, np.arange(W) - (W - 1) / 2.0, indexing='ij')
    out = np.empty(shape, dtype=np.float64).reshape(-1, H, W)
    for img in out:
        cy, cx = rng.uniform(-0.15, 0.15, 2) * (H, W)
        sy, sx = rng.uniform(0.04, 0.07, 2) * (H, W)            # compact: no baseline resolves it out
        img[:] = np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
        img += 0.05 * rng.uniform(size=(H, W))
        img *= 2.0 / img.sum()
    return out.reshape(shape).astype(np.float32)


def dense128(uv, fov, H, W):
    """observation.dft_matrix's formula in complex128 for H x W pixels: (B, nvis, H W)."""
    x = (np.arange(W) - (W - 1) / 2.0) * (fov / W)
    y = (np.arange(H) - (H - 1) / 2.0) * (fov / H)
    yy, xx = np.meshgrid(y, x, indexing='ij')
    return np.exp(1j * (-2.0 * np.pi * (uv[..., 0:1] * xx.reshape(-1) + uv[..., 1:2] * yy.reshape(-1))))


def table_loss(images, A, target, sigma, scale, dtype, tri=None, sign=None):
    """float64 loss and d loss / d images of the table form.  images (B, [S,] H, W); A (B, nvis, R) complex128; target / sigma
    (B, [S,] nvis | ncp).  Returns (loss, grad shaped like images, visibilities (B, [S,] nvis) complex128)."""
    img = torch.tensor(np.asarray(images, dtype=np.float64), requires_grad=True)
    At = torch.tensor(A)
    B = img.shape[0]
    vec = img.reshape(B, -1, img.shape[-2] * img.shape[-1]).to(torch.complex128)             # (B, S, R)
    vis = torch.einsum('bkr,bsr->bsk', At, vec).reshape(tuple(img.shape[:-2]) + (A.shape[1],))
    tg, sg = torch.tensor(np.asarray(target)), torch.tensor(np.asarray(sigma, dtype=np.float64))
    if dtype == 'vis':
        loss = scale * (((vis - tg.to(torch.complex128)).abs() / sg) ** 2).sum()
    elif dtype == 'amp':
        loss = scale * (((vis.abs() - tg.to(torch.float64)) / sg) ** 2).sum()
    else:
        bis = 1.0
        for leg in range(3):
            v = vis[..., torch.tensor(tri[:, leg].astype(np.int64))]
            bis = bis * torch.where(torch.tensor(sign[:, leg] < 0), v.conj(), v)
        loss = scale * ((1.0 - torch.cos(tg.to(torch.float64) - torch.angle(bis))) / sg ** 2).sum()
    loss.backward()
    return loss.item(), img.grad.numpy(), vis.detach().numpy()


def closure_phases(vis, tri, sign):
    bis = 1.0
    for leg in range(3):
        v = vis[..., tri[:, leg]]
        bis = bis * np.where(sign[:, leg] < 0, np.conj(v), v)
    return np.angle(bis)


_CASES = {}


def case(name, Sx=0, spec=None, fov=FOV):
    """Everything about one input set, computed once and left unchanged: a dict with the operator pieces (uv, pairs, triangles,
    tri, sign), images (B, [Sx,] H, W) float32, per dtype (target, sigma) and the float64 reference (loss, grad, vis) at scale 1.
    spec: an explicit (H, W, B, seed, stations) under a name of the caller's instead of a row of CASES (tests/eht_edge_cases.py);
    fov: the field of view, for such a case."""
    key = (name, Sx) if spec is None else (name, Sx, tuple(spec), fov)
    if key in _CASES:
        return _CASES[key]
    H, W, B, seed, ns = spec if spec is not None else BIG if name == 'big' else CASES[name]
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(B, ns, 2)) * 3e9
    pairs = np.array([(i, j) for i in range(ns) for j in range(i + 1, ns)])
    uv = np.ascontiguousarray(pos[:, pairs[:, 0]] - pos[:, pairs[:, 1]])                     # (B, nvis, 2) float64
    triangles = observation.closure_triangles(ns)
    tri, sign = observation.closure_table(pairs, triangles)
    shape = (B, Sx, H, W) if Sx else (B, H, W)
    images, truth = blobs(rng, shape), blobs(rng, shape)
    A = dense128(uv, fov, H, W)
    vis_truth = table_loss(truth, A, np.zeros(shape[:-2] + (len(pairs),), dtype=np.complex128), 1.0, 1.0, 'vis')[2]
    s_vis = (0.05 * np.abs(vis_truth).mean() * rng.uniform(0.5, 1.5, vis_truth.shape)).astype(np.float32)
    cp = closure_phases(vis_truth, tri, sign)
    data = {'vis': (vis_truth.astype(np.complex64), s_vis),
            'amp': (np.abs(vis_truth).astype(np.float32), s_vis),
            'cphase': (cp.astype(np.float32), rng.uniform(0.05, 0.2, cp.shape).astype(np.float32))}
    ref = {d: table_loss(images, A, t, s, 1.0, d, tri, sign) for d, (t, s) in data.items()}
    amp = np.abs(ref['vis'][2])
    out = dict(name=name, H=H, W=W, B=B, ns=ns, Sx=Sx, uv=uv, pairs=pairs, triangles=triangles, tri=tri, sign=sign, images=images,
               data=data, ref=ref, A128=A, min_amp=float(amp.min() / amp.max()), fov=fov)
    _CASES[key] = out
    return out


def operator(c, dtype):
    """The DirectDFT of a case for one dtype: with the triangle table for 'cphase', without otherwise."""
    if dtype == 'cphase':
        return observation.DirectDFT(c['uv'], c.get('fov', FOV), (c['H'], c['W']), triangles=c['triangles'], pairs=c['pairs'])
    return observation.DirectDFT(c['uv'], c.get('fov', FOV), (c['H'], c['W']))


def rel_max(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())
