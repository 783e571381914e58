"""Visibility-domain measurement operators for the EHT losses (reference: bhnerf/observation.py wraps
ehtim, an external package).  Only what the hot path consumes is provided: the direct-DFT matrix
``A[k, p] = exp(-2 pi i (u_k x_p + v_k y_p))`` that maps an image vector to complex visibilities, in the
shape ``loss_fn_eht`` expects (network.py:541-544).  Not a re-implementation of ehtim's pulse functions or
its sign/ordering conventions (parity unpinned: SURVEY 8c iii).

``DirectDFT`` is the same operator kept as its (u, v) coordinates: the losses then run matrix-free (libbhnerf_eht.so).
``ClosureDFT`` is a ``DirectDFT`` with the closure tables (triangles, quadrangles) and weights of one combined objective over
'amp', 'cphase' and 'logcamp', the log closure amplitude (libbhnerf_cls.so)."""
import numpy as np


def dft_matrix(uv, fov, npix):
    """uv: (nvis, 2) baselines in wavelengths; fov: field of view in radians; npix: image is npix x npix
    (row-major, H then W as flattened by loss_fn_eht).  Returns complex64 (nvis, npix*npix)."""
    uv = np.asarray(uv, dtype=np.float64)
    x = (np.arange(npix) - (npix - 1) / 2.0) * (fov / npix)
    yy, xx = np.meshgrid(x, x, indexing='ij')
    phase = -2.0 * np.pi * (uv[:, 0:1] * xx.reshape(1, -1) + uv[:, 1:2] * yy.reshape(1, -1))
    return np.exp(1j * phase).astype(np.complex64)


def closure_triangles(nsites):
    """All site triples (i<j<k) of an array with nsites stations."""
    return [(i, j, k) for i in range(nsites) for j in range(i + 1, nsites) for k in range(j + 1, nsites)]


def closure_table(pairs, triangles):
    """The closure-phase index table of ``bhn_eht_chi2_uv``: for each station triple (a, b, c) the baselines of the legs
    (a, b), (b, c) and conj (a, c) -- the legs ``tests/test_gpu_eht2017.py`` builds dense matrices for.  ``pairs`` (nvis, 2)
    names the stations of each stored baseline; a baseline stored as (j, i) serves the leg (i, j) with the opposite sign.
    Returns ``tri`` (ncp, 3) int32 and ``tri_sign`` (ncp, 3) int8 (+1: the visibility as stored, -1: its conjugate);
    ValueError when a leg has no baseline."""
    index = {}
    for i, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        index.setdefault((a, b), (i, 1))
        index.setdefault((b, a), (i, -1))
    triangles = np.asarray(triangles).reshape(-1, 3).tolist()
    tri = np.zeros((len(triangles), 3), dtype=np.int32)
    sign = np.zeros((len(triangles), 3), dtype=np.int8)
    for c, (a, b, d) in enumerate(triangles):
        for leg, (p, q, s) in enumerate(((a, b, 1), (b, d, 1), (a, d, -1))):
            if (p, q) not in index:
                raise ValueError('triangle {} needs the baseline ({}, {}), which is not in pairs'.format((a, b, d), p, q))
            tri[c, leg], sign[c, leg] = index[(p, q)][0], s * index[(p, q)][1]
    return tri, sign


class DirectDFT(object):
    """The direct-DFT measurement operator of the EHT losses as what it is made of: the (u, v) coordinates.

    ``uv``: (nt, nvis, 2) float64, wavelengths; ``fov``: radians, one number for both axes or (fov_y, fov_x); ``npix``: an int or
    (H, W) -- pixel (y, x) sits at ((x - (W - 1) / 2) fov_x / W, (y - (H - 1) / 2) fov_y / H), as in ``dft_matrix``.
    ``triangles``: closure phases -- station triples together with ``pairs`` (nvis, 2), or a ready ``(tri, tri_sign)`` table
    (``closure_table``).  Pass the object wherever ``loss_fn_eht``, ``gradient_step_eht``, ``test_eht``, ``engine.chi2_eht`` or
    ``TrainStep.eht_arrays`` take the dense matrices ``A``: the loss then runs from the coordinates (libbhnerf_eht.so) and no
    (nvis, H W) matrix is ever built.  ``uv`` stays float64, on the host and on the device."""

    def __init__(self, uv, fov, npix, triangles=None, pairs=None):
        import torch
        if isinstance(uv, torch.Tensor):
            if uv.dtype != torch.float64:
                raise AttributeError('uv must be float64 (got {})'.format(uv.dtype))
            self.uv = uv.contiguous()
        else:
            self.uv = np.ascontiguousarray(np.asarray(uv, dtype=np.float64))
        if self.uv.ndim != 3 or self.uv.shape[-1] != 2:
            raise AttributeError('uv should have the shape (nt, nvis, 2), got {}'.format(tuple(self.uv.shape)))
        self.H, self.W = (int(npix), int(npix)) if np.ndim(npix) == 0 else (int(npix[0]), int(npix[1]))
        self.fov = (float(fov), float(fov)) if np.ndim(fov) == 0 else (float(fov[0]), float(fov[1]))
        if self.H < 1 or self.W < 1 or not (self.fov[0] > 0 and self.fov[1] > 0):
            raise AttributeError('npix and fov must be positive')
        self.tri = self.tri_sign = None
        if triangles is not None:
            if pairs is not None:
                tri, sign = closure_table(pairs, triangles)
            else:
                tri, sign = triangles
            keep = isinstance(tri, torch.Tensor)                # (a table already on the device: .take / .to hand it on)
            t = tri.cpu().numpy() if keep else np.asarray(tri)
            s = sign.cpu().numpy() if keep else np.asarray(sign)
            if t.ndim != 2 or t.shape[1] != 3 or s.shape != t.shape or t.shape[0] < 1:
                raise AttributeError('the closure table should be (ncp, 3) indices and (ncp, 3) signs')
            if t.min() < 0 or t.max() >= self.nvis or not np.isin(s, (-1, 1)).all():
                raise AttributeError('closure table: baseline indices must lie in [0, {}) and signs be +-1'.format(self.nvis))
            self.tri = tri.to(torch.int32).contiguous() if keep else np.ascontiguousarray(t, dtype=np.int32)
            self.tri_sign = sign.to(torch.int8).contiguous() if keep else np.ascontiguousarray(s, dtype=np.int8)

    # -- what TemporalBatchedArgs needs of a per-frame argument
    @property
    def shape(self):
        return tuple(self.uv.shape)

    @property
    def nvis(self):
        return int(self.uv.shape[1])

    @property
    def ncp(self):
        return 0 if self.tri is None else int(self.tri.shape[0])

    @property
    def psize(self):
        """(psize_y, psize_x) in radians."""
        return self.fov[0] / self.H, self.fov[1] / self.W

    def _like(self, uv, tri=None, tri_sign=None):
        out = object.__new__(DirectDFT)
        out.uv, out.H, out.W, out.fov = uv, self.H, self.W, self.fov
        out.tri, out.tri_sign = (self.tri, self.tri_sign) if tri is None else (tri, tri_sign)
        return out

    def to(self, device):
        """The operator with ``uv`` (float64) and the closure table on ``device``."""
        import torch
        mv = lambda a: None if a is None else torch.as_tensor(a, device=device)
        return self._like(mv(self.uv), mv(self.tri), mv(self.tri_sign))

    def take(self, indices):
        """The operator of a batch of frames: on a device an ``index_select`` of the float64 ``uv``."""
        import torch
        if isinstance(self.uv, torch.Tensor):
            idx = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices, dtype=np.int64), device=self.uv.device)
            return self._like(self.uv.index_select(0, idx.to(device=self.uv.device, dtype=torch.int64)))
        idx = indices.cpu().numpy() if isinstance(indices, torch.Tensor) else np.asarray(indices)
        return self._like(np.ascontiguousarray(self.uv[idx]))

    def dense(self, dtype=np.complex64):
        """The dense matrices this operator stands for: (nt, nvis, H W), what stacking ``dft_matrix`` per frame gives, or with
        triangles (nt, 3, ncp, H W), the three legs of each closure phase with the conjugated ones conjugated."""
        import torch
        uv = self.uv.cpu().numpy() if isinstance(self.uv, torch.Tensor) else self.uv
        x = (np.arange(self.W) - (self.W - 1) / 2.0) * (self.fov[1] / self.W)
        y = (np.arange(self.H) - (self.H - 1) / 2.0) * (self.fov[0] / self.H)
        yy, xx = np.meshgrid(y, x, indexing='ij')
        A = np.stack([np.exp(1j * (-2.0 * np.pi * (f[:, 0:1] * xx.reshape(1, -1) + f[:, 1:2] * yy.reshape(1, -1)))).astype(dtype)
                      for f in uv])
        if self.tri is None:
            return A
        tri = self.tri.cpu().numpy() if isinstance(self.tri, torch.Tensor) else self.tri
        sign = self.tri_sign.cpu().numpy() if isinstance(self.tri_sign, torch.Tensor) else self.tri_sign
        legs = [np.where((sign[:, leg] < 0)[None, :, None], np.conj(A[:, tri[:, leg]]), A[:, tri[:, leg]]) for leg in range(3)]
        return np.stack(legs, axis=1)

    def observe(self, movie, device=None):
        """Complex visibilities (nt, [S,] nvis) of ``movie`` (nt, [S,] H, W) as a complex64 device tensor (``bhn_eht_vis``).
        Runs on the HIP device only: ``HipError`` without one."""
        import torch
        from . import _hip, engine
        if not torch.cuda.is_available():
            raise _hip.HipError('DirectDFT.observe runs on the HIP device only (no CPU fallback; .dense() gives the matrices)')
        if isinstance(self.uv, torch.Tensor) and self.uv.is_cuda:
            op = self
        else:
            op = self.to(torch.device(device if device is not None else 'cuda'))
        movie = _hip.as_f32(movie, op.uv.device)
        return engine.eht_vis_uv(movie, op)


CLOSURE_TERMS = ('amp', 'cphase', 'logcamp')         # the canonical order of the terms of a combined closure loss


def closure_quadrangles(nsites):
    """The independent log closure amplitudes of every station quadruple a<b<c<d of an array with nsites stations, two per
    quadruple: (ab cd | ac bd) and (ad bc | ac bd).  Returns (nca, 4, 2) station pairs: legs 0 and 1 the numerator, legs 2 and 3
    the denominator."""
    rows = []
    for a in range(nsites):
        for b in range(a + 1, nsites):
            for c in range(b + 1, nsites):
                for d in range(c + 1, nsites):
                    rows.append(((a, b), (c, d), (a, c), (b, d)))
                    rows.append(((a, d), (b, c), (a, c), (b, d)))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4, 2)


def quadrangle_table(pairs, quadrangles):
    """The log-closure-amplitude index table of ``bhn_cls_chi2``: for each quadrangle (four station pairs, ``closure_quadrangles``)
    the baselines of its legs.  ``pairs`` (nvis, 2) names the stations of each stored baseline; amplitudes do not see the
    orientation, so a baseline stored as (j, i) serves the leg (i, j).  Returns (nca, 4) int32; ValueError when a leg has no
    baseline."""
    index = {}
    for i, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        index.setdefault((a, b), i)
        index.setdefault((b, a), i)
    quadrangles = np.asarray(quadrangles).reshape(-1, 4, 2).tolist()
    quad = np.zeros((len(quadrangles), 4), dtype=np.int32)
    for q, legs in enumerate(quadrangles):
        for leg, (a, b) in enumerate(legs):
            if (a, b) not in index:
                raise ValueError('quadrangle {} needs the baseline ({}, {}), which is not in pairs'.format(
                    tuple(tuple(l) for l in legs), a, b))
            quad[q, leg] = index[(a, b)]
    return quad


class ClosureDFT(DirectDFT):
    """A ``DirectDFT`` that carries the closure tables of ONE weighted objective over the real-valued terms 'amp', 'cphase' and
    'logcamp' (libbhnerf_cls.so): one render, one visibility pass and one gradient for ``scale * sum_d w_d chi^2_d``.

    ``triangles`` / ``quadrangles``: station triples / quadrangles of station pairs (``closure_triangles``,
    ``closure_quadrangles``) together with ``pairs`` (nvis, 2), or without ``pairs`` the ready tables ``(tri, tri_sign)`` and
    ``quad`` (nca, 4).  ``weights``: {'amp' | 'cphase' | 'logcamp': w_d >= 0}, 1.0 where not given.  The data of a combined dtype
    such as 'cphase+logcamp' are the terms' arrays concatenated along the last axis in the canonical order (``pack``)."""

    def __init__(self, uv, fov, npix, pairs=None, triangles=None, quadrangles=None, weights=None):
        import torch
        DirectDFT.__init__(self, uv, fov, npix, triangles=triangles, pairs=pairs if triangles is not None else None)
        self.quad = None
        if quadrangles is not None:
            quad = quadrangle_table(pairs, quadrangles) if pairs is not None else quadrangles
            keep = isinstance(quad, torch.Tensor)
            q = quad.cpu().numpy() if keep else np.asarray(quad)
            if q.ndim != 2 or q.shape[1] != 4 or q.shape[0] < 1:
                raise AttributeError('the quadrangle table should be (nca, 4) baseline indices')
            if q.min() < 0 or q.max() >= self.nvis:
                raise AttributeError('quadrangle table: baseline indices must lie in [0, {})'.format(self.nvis))
            self.quad = quad.to(torch.int32).contiguous() if keep else np.ascontiguousarray(q, dtype=np.int32)
        self.weights = self._weights(weights)

    @staticmethod
    def _weights(weights):
        weights = dict(weights or {})
        unknown = sorted(set(weights) - set(CLOSURE_TERMS))
        if unknown:
            raise AttributeError('weights name unknown terms {} (known: {})'.format(unknown, ', '.join(CLOSURE_TERMS)))
        out = {k: float(weights.get(k, 1.0)) for k in CLOSURE_TERMS}
        if not all(np.isfinite(w) and w >= 0 for w in out.values()):
            raise AttributeError('weights must be finite and >= 0, got {}'.format(out))
        return out

    @property
    def nca(self):
        return 0 if self.quad is None else int(self.quad.shape[0])

    def term_sizes(self):
        """{term: entries along the last axis} of the terms this operator has a table for ('amp' needs none)."""
        sizes = {'amp': self.nvis}
        if self.tri is not None:
            sizes['cphase'] = self.ncp
        if self.quad is not None:
            sizes['logcamp'] = self.nca
        return sizes

    def _like(self, uv, tri=None, tri_sign=None, quad=None):
        out = object.__new__(type(self))
        out.uv, out.H, out.W, out.fov = uv, self.H, self.W, self.fov
        out.tri, out.tri_sign = (self.tri, self.tri_sign) if tri is None else (tri, tri_sign)
        out.quad = self.quad if quad is None else quad
        out.weights = dict(self.weights)
        return out

    def to(self, device):
        """The operator with ``uv`` (float64) and the closure tables on ``device``."""
        import torch
        mv = lambda a: None if a is None else torch.as_tensor(a, device=device)
        return self._like(mv(self.uv), mv(self.tri), mv(self.tri_sign), mv(self.quad))

    @staticmethod
    def _host(a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def closure_phases(self, vis):
        """float64 closure phases (..., ncp) in radians of complex visibilities (..., nvis), through the triangle table."""
        if self.tri is None:
            raise AttributeError('closure phases need a ClosureDFT with triangles')
        vis = np.asarray(vis, dtype=np.complex128)
        tri, sign = self._host(self.tri), self._host(self.tri_sign)
        bis = 1.0
        for leg in range(3):
            v = vis[..., tri[:, leg]]
            bis = bis * np.where(sign[:, leg] < 0, np.conj(v), v)
        return np.angle(bis)

    def log_closure_amplitudes(self, vis):
        """float64 log closure amplitudes (..., nca) of complex visibilities (..., nvis), through the quadrangle table."""
        if self.quad is None:
            raise AttributeError('log closure amplitudes need a ClosureDFT with quadrangles')
        logamp = np.log(np.abs(np.asarray(vis, dtype=np.complex128)))
        quad = self._host(self.quad)
        return logamp[..., quad[:, 0]] + logamp[..., quad[:, 1]] - logamp[..., quad[:, 2]] - logamp[..., quad[:, 3]]

    def pack(self, data):
        """{'cphase': x, 'logcamp': y, ...} -> the arrays concatenated along the last axis in the canonical order (amp, cphase,
        logcamp; only the terms named)."""
        sizes = self.term_sizes()
        parts = []
        unknown = sorted(set(data) - set(CLOSURE_TERMS))
        if unknown or not data:
            raise AttributeError('pack takes terms of {}, got {}'.format(CLOSURE_TERMS, sorted(data)))
        for name in CLOSURE_TERMS:
            if name in data:
                x = np.asarray(data[name])
                if name not in sizes or x.shape[-1] != sizes[name]:
                    raise AttributeError("term '{}' of shape {} does not end in the operator's {} entries".format(
                        name, x.shape, sizes.get(name, 0)))
                parts.append(x)
        return np.concatenate(parts, axis=-1)

    def split(self, array, terms=None):
        """The inverse of ``pack``: {term: its slice of the last axis}.  ``terms``: the names (any iterable, or a '+'-joined string);
        None: the one set of this operator's terms whose sizes add up to the last axis."""
        sizes = self.term_sizes()
        n = int(array.shape[-1])
        if terms is None:
            from itertools import combinations
            fits = [c for r in range(1, len(sizes) + 1) for c in combinations([t for t in CLOSURE_TERMS if t in sizes], r)
                    if sum(sizes[t] for t in c) == n]
            if len(fits) != 1:
                raise AttributeError('a last axis of {} entries names {} sets of terms of {}: pass terms'.format(n, len(fits), sizes))
            terms = fits[0]
        elif isinstance(terms, str):
            terms = terms.split('+')
        terms = [t for t in CLOSURE_TERMS if t in set(terms)]
        if not terms or any(t not in sizes for t in terms) or sum(sizes[t] for t in terms) != n:
            raise AttributeError('a last axis of {} entries is not the terms {} of {}'.format(n, terms, sizes))
        out, o = {}, 0
        for t in terms:
            out[t] = array[..., o:o + sizes[t]]
            o += sizes[t]
        return out
