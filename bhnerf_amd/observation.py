"""Visibility-domain measurement operators for the EHT losses (reference: bhnerf/observation.py wraps
ehtim, an external package).  Only what the hot path consumes is provided: the direct-DFT matrix
``A[k, p] = exp(-2 pi i (u_k x_p + v_k y_p))`` that maps an image vector to complex visibilities, in the
shape ``loss_fn_eht`` expects (network.py:541-544).  Not a re-implementation of ehtim's pulse functions or
its sign/ordering conventions (parity unpinned: SURVEY 8c iii).

``DirectDFT`` is the same operator kept as its (u, v) coordinates: the losses then run matrix-free (libbhnerf_eht.so).
``ClosureDFT`` is a ``DirectDFT`` with the closure tables (triangles, quadrangles) and weights of one combined objective over
'amp', 'cphase' and 'logcamp', the log closure amplitude (libbhnerf_cls.so).  ``PolDFT`` is a ``DirectDFT`` for the polarimetric
terms that couple the Stokes planes of a frame: 'pvis', P = Q + iU, and 'm', the visibility-domain fractional polarisation P / I
(libbhnerf_pol.so).

``Array``, ``empty_eht_obs``, ``observe_same`` and ``Observation`` lead from a station table to those operators: baseline
coordinates, elevations, thermal noise, synthetic visibilities and the targets, sigmas and closure tables of a station set that
changes from frame to frame -- what the reference asks of ehtim (observation.py:79-222), in NumPy float64 on the host."""
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

    def _like(self, uv, move=None):
        """The operator on another ``uv``, with whatever of the tables and weights this one has (a subclass adds ``quad``,
        ``weights``); ``move``: what takes a table to where ``uv`` now is (None: the tables as they are)."""
        out = object.__new__(type(self))
        out.uv, out.H, out.W, out.fov = uv, self.H, self.W, self.fov
        for k in ('tri', 'tri_sign', 'quad'):
            if hasattr(self, k):
                table = getattr(self, k)
                setattr(out, k, table if table is None or move is None else move(table))
        if hasattr(self, 'weights'):
            out.weights = dict(self.weights)
        return out

    def to(self, device):
        """The operator with ``uv`` (float64) and the closure tables on ``device``."""
        import torch
        mv = lambda a: torch.as_tensor(a, device=device)
        return self._like(mv(self.uv), mv)

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


def term_weights(canonical, weights, default):
    """{term: w >= 0} over the terms ``canonical`` from ``weights`` ({term: w} or None), ``default`` where not given;
    AttributeError for an unknown term and for a weight that is negative or not finite."""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(canonical))
    if unknown:
        raise AttributeError('weights name unknown terms {} (known: {})'.format(unknown, ', '.join(canonical)))
    out = {k: float(weights.get(k, default)) for k in canonical}
    if not all(np.isfinite(w) and w >= 0 for w in out.values()):
        raise AttributeError('weights must be finite and >= 0, got {}'.format(out))
    return out


class TermSet(object):
    """What the operators of ONE weighted objective ``scale * sum_d w_d chi^2_d`` share (a mixin): ``TERMS``, the canonical order
    of the terms, and ``term_sizes()``, {term: entries along the last axis} of the terms the operator can serve, give the weights
    and the layout of the data -- the terms' arrays concatenated along the last axis in the canonical order."""
    TERMS = ()

    def _weights(self, weights, default=1.0):
        return term_weights(self.TERMS, weights, default)

    def pack(self, data):
        """{term: x, ...} -> the arrays concatenated along the last axis in the canonical order (only the terms named)."""
        sizes = self.term_sizes()
        unknown = sorted(set(data) - set(self.TERMS))
        if unknown or not data:
            raise AttributeError('pack takes terms of {}, got {}'.format(self.TERMS, sorted(data)))
        parts = []
        for name in self.TERMS:
            if name in data:
                x = np.asarray(data[name])
                if name not in sizes or x.ndim < 1 or x.shape[-1] != sizes[name]:
                    raise AttributeError("term '{}' of shape {} does not end in the operator's {} entries".format(
                        name, x.shape, sizes.get(name, 0)))
                parts.append(x)
        return np.concatenate(parts, axis=-1)

    def split(self, array, terms=None):
        """The inverse of ``pack``: {term: its slice of the last axis}.  ``terms``: the names (any iterable, or a '+'-joined string);
        None: the one set of this operator's terms whose sizes add up to the last axis (terms of equal size have to be named)."""
        sizes = self.term_sizes()
        n = int(array.shape[-1])
        if terms is None:
            from itertools import combinations
            fits = [c for r in range(1, len(sizes) + 1) for c in combinations([t for t in self.TERMS if t in sizes], r)
                    if sum(sizes[t] for t in c) == n]
            if len(fits) != 1:
                raise AttributeError('a last axis of {} entries names {} sets of terms of {}: pass terms'.format(n, len(fits), sizes))
            terms = fits[0]
        elif isinstance(terms, str):
            terms = terms.split('+')
        terms = [t for t in self.TERMS if t in set(terms)]
        if not terms or any(t not in sizes for t in terms) or sum(sizes[t] for t in terms) != n:
            raise AttributeError('a last axis of {} entries is not the terms {} of {}'.format(n, terms, sizes))
        out, o = {}, 0
        for t in terms:
            out[t] = array[..., o:o + sizes[t]]
            o += sizes[t]
        return out


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


class ClosureDFT(TermSet, DirectDFT):
    """A ``DirectDFT`` that carries the closure tables of ONE weighted objective over the real-valued terms 'amp', 'cphase' and
    'logcamp' (libbhnerf_cls.so): one render, one visibility pass and one gradient for ``scale * sum_d w_d chi^2_d``.

    ``triangles`` / ``quadrangles``: station triples / quadrangles of station pairs (``closure_triangles``,
    ``closure_quadrangles``) together with ``pairs`` (nvis, 2), or without ``pairs`` the ready tables ``(tri, tri_sign)`` and
    ``quad`` (nca, 4).  ``weights``: {'amp' | 'cphase' | 'logcamp': w_d >= 0}, 1.0 where not given.  The data of a combined dtype
    such as 'cphase+logcamp' are the terms' arrays concatenated along the last axis in the canonical order (``pack``)."""
    TERMS = CLOSURE_TERMS

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


POL_TERMS = ('pvis', 'm')                           # the canonical order of the polarimetric terms


class PolDFT(TermSet, DirectDFT):
    """A ``DirectDFT`` for ONE weighted objective over the polarimetric terms 'pvis' and 'm' (libbhnerf_pol.so), which couple the
    Stokes planes I, Q, U[, V] of a frame: with P = Q~ + i U~ per frame and baseline,

    'pvis': |P - target|^2 / sigma^2, the calibrated polarised visibility; 'm': |P / I~ - target|^2 / sigma^2, the fractional
    polarisation in the visibility domain.  A complex station gain G_a conj(G_b) common to the Stokes planes of a baseline
    multiplies P and I~ alike, so 'm' does not see it: the polarimetric counterpart of the closure quantities.

    ``weights``: {'pvis' | 'm': w_d >= 0}, 1.0 where not given.  Targets are complex (nt, nvis), sigmas real (nt, nvis) -- one per
    frame and baseline, not per plane; the data of 'pvis+m' are the terms' arrays concatenated along the last axis in the
    canonical order (``pack``; ``split`` without names takes a last axis of 2 nvis entries only: 'pvis' and 'm' have the same
    size).  ``observe`` is ``DirectDFT``'s."""
    TERMS = POL_TERMS

    def __init__(self, uv, fov, npix, weights=None):
        DirectDFT.__init__(self, uv, fov, npix)
        self.weights = self._weights(weights)

    def term_sizes(self):
        """{term: entries along the last axis}: one per baseline for either term."""
        return {t: self.nvis for t in POL_TERMS}

    @staticmethod
    def _planes(vis):
        vis = np.asarray(vis, dtype=np.complex128)
        if vis.ndim < 2 or vis.shape[-2] < 3:
            raise AttributeError('polarimetric quantities need visibilities (..., S >= 3, nvis) of the planes I, Q, U; got {}'.format(vis.shape))
        return vis

    def polarised_visibility(self, vis):
        """complex128 P = Q~ + i U~ (..., nvis) of complex visibilities (..., S >= 3, nvis) of the planes I, Q, U[, V]."""
        vis = self._planes(vis)
        return vis[..., 1, :] + 1j * vis[..., 2, :]

    def fractional_polarisation(self, vis):
        """complex128 P / I~ (..., nvis) of complex visibilities (..., S >= 3, nvis); inf or NaN where I~ is zero."""
        vis = self._planes(vis)
        with np.errstate(divide='ignore', invalid='ignore'):
            return (vis[..., 1, :] + 1j * vis[..., 2, :]) / vis[..., 0, :]


# ---------------------------------------------------------------------------------------------------------------------------
# From a station table to what the operators above take: baseline coordinates, thermal noise and per-frame closure tables of an
# earth-rotation synthesis (reference: observation.py:79-119 and 121-222 hand this to ehtim).  NumPy float64 on the host.
# ---------------------------------------------------------------------------------------------------------------------------
C_LIGHT = 299792458.0            # m / s
QUANT_EFFICIENCY = 0.88          # 2-bit quantisation, the factor of the thermal noise of one baseline


class Array(object):
    """A station table: ``names`` (nsites,), ``xyz`` (nsites, 3) earth-fixed metres, ``sefd`` (nsites,) Jy."""

    def __init__(self, names, xyz, sefd):
        self.names = [str(n) for n in names]
        self.xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64))
        self.sefd = np.ascontiguousarray(np.asarray(sefd, dtype=np.float64))
        n = len(self.names)
        if n < 2 or self.xyz.shape != (n, 3) or self.sefd.shape != (n,):
            raise AttributeError('an Array takes n >= 2 names, xyz (n, 3) and sefd (n,); got {} names, xyz {}, sefd {}'.format(
                n, self.xyz.shape, self.sefd.shape))
        if not (np.isfinite(self.xyz).all() and np.isfinite(self.sefd).all() and (self.sefd > 0).all()):
            raise AttributeError('station coordinates must be finite and SEFDs finite and positive')

    @classmethod
    def load_txt(cls, path):
        """A table in the text format of ehtim's arrays: '#' lines and blank lines are skipped, the columns are
        ``NAME X Y Z SEFDR [SEFDL ...]`` (further columns ignored).  The station's SEFD is (SEFDR + SEFDL) / 2, SEFDL = SEFDR when
        the table has no such column."""
        names, xyz, sefd = [], [], []
        with open(path) as f:
            for line in f:
                col = line.split()
                if not col or col[0].startswith('#'):
                    continue
                if len(col) < 5:
                    raise AttributeError('{}: a station line needs NAME X Y Z SEFDR, got {!r}'.format(path, line.rstrip()))
                names.append(col[0])
                xyz.append([float(v) for v in col[1:4]])
                sefd.append(0.5 * (float(col[4]) + float(col[5] if len(col) > 5 else col[4])))
        return cls(names, xyz, sefd)

    def __len__(self):
        return len(self.names)

    @property
    def pairs(self):
        """Every station pair i < j: (nsites (nsites - 1) / 2, 2)."""
        n = len(self)
        return np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int64)


def utc_to_gmst(mjd, utc_hours):
    """Greenwich mean sidereal time in hours [0, 24) at ``utc_hours`` of the day ``mjd``: the IAU-1982 linear form
    18.697374558 + 24.06570982441908 D, D the days from JD 2451545.0, with UT1 = UTC."""
    D = (np.asarray(mjd, dtype=np.float64) - 51544.5) + np.asarray(utc_hours, dtype=np.float64) / 24.0
    return np.mod(18.697374558 + 24.06570982441908 * D, 24.0)


def empty_eht_obs(array, nt, tint, tstart=4.0, tstop=15.5, ra=17.761121055553343, dec=-29.00784305556, rf=226191789062.5,
                  mjd=57850, bw=1856000000.0, timetype='UTC', polrep='stokes', *, times=None, elev_min=10.0, elev_max=85.0):
    """The empty observation of ``array`` (an ``Array``) on a source: baseline coordinates, elevations and thermal noise of ``nt``
    scans -- the reference's name, argument order and defaults (observation.py:79), so its ``obs_params`` works with only 'array'
    changed.  ``tint``: integration time in seconds; ``tstart`` / ``tstop``: hours, scan k at tstart + k (tstop - tstart) / nt;
    ``times`` (hours) overrides that grid; ``ra``: hours, ``dec``: degrees; ``rf``, ``bw``: Hz; ``timetype``: 'UTC' (converted with
    ``utc_to_gmst`` on the day ``mjd``) or 'GMST' (the times are Greenwich mean sidereal hours).  ``polrep``: 'stokes' only.

    Baselines are all station pairs i < j.  (u, v) in wavelengths c / rf by the closed form of Thompson, Moran & Swenson eq. 4.1
    for the baseline vector xyz_j - xyz_i; elevation arcsin(s . r) per station with r the geocentric unit vector; a baseline is
    ``up`` when both stations lie strictly between ``elev_min`` and ``elev_max`` degrees; thermal noise
    sigma_ij = sqrt(sefd_i sefd_j / (2 bw tint)) / 0.88.

    Not ehtim: no precession or nutation, no geodetic latitude, UT1 = UTC, and none of ehtim's scan bookkeeping (tadv rounding,
    time-sorted records, conjugate ordering) -- parity with ``ehtim.Array.obsdata`` is NOT pinned."""
    if not isinstance(array, Array):
        raise AttributeError('array should be an observation.Array (Array.load_txt(path)), got {}'.format(type(array).__name__))
    if polrep != 'stokes':
        raise AttributeError("polrep ({}) not supported: 'stokes' only".format(polrep))
    if timetype not in ('UTC', 'GMST'):
        raise AttributeError("timetype ({}) should be 'UTC' or 'GMST'".format(timetype))
    if times is None:
        if int(nt) < 1:
            raise AttributeError('nt must be at least 1')
        times = float(tstart) + np.arange(int(nt)) * ((float(tstop) - float(tstart)) / int(nt))
    times = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if times.ndim != 1 or times.size != int(nt):
        raise AttributeError('times should hold nt = {} hours, got the shape {}'.format(nt, times.shape))
    if not (tint > 0 and bw > 0 and rf > 0):
        raise AttributeError('tint, bw and rf must be positive')
    gmst = np.mod(times, 24.0) if timetype == 'GMST' else utc_to_gmst(mjd, times)
    pairs = array.pairs
    lam = C_LIGHT / float(rf)
    H = (gmst - float(ra)) * (np.pi / 12.0)                                # Greenwich hour angle of the source
    d = np.deg2rad(float(dec))
    B = array.xyz[pairs[:, 1]] - array.xyz[pairs[:, 0]]                    # earth-fixed baseline vectors (m)
    sH, cH = np.sin(H)[:, None], np.cos(H)[:, None]
    u = (sH * B[None, :, 0] + cH * B[None, :, 1]) / lam
    v = (-np.sin(d) * cH * B[None, :, 0] + np.sin(d) * sH * B[None, :, 1] + np.cos(d) * B[None, :, 2]) / lam
    # the source direction in the earth-fixed frame (hour angle H west of Greenwich) against each station's geocentric direction
    s = np.stack([np.cos(d) * np.cos(-H), np.cos(d) * np.sin(-H), np.full_like(H, np.sin(d))], axis=-1)
    rhat = array.xyz / np.linalg.norm(array.xyz, axis=1, keepdims=True)
    elevation = np.arcsin(np.clip(s @ rhat.T, -1.0, 1.0))
    site_up = (elevation > np.deg2rad(elev_min)) & (elevation < np.deg2rad(elev_max))
    up = site_up[:, pairs[:, 0]] & site_up[:, pairs[:, 1]]
    sigma = np.sqrt(array.sefd[pairs[:, 0]] * array.sefd[pairs[:, 1]] / (2.0 * float(bw) * float(tint))) / QUANT_EFFICIENCY
    return Observation(array, times, gmst, pairs, np.stack([u, v], axis=-1), up, np.broadcast_to(sigma, up.shape).copy(), elevation,
                       ra=float(ra), dec=float(dec), rf=float(rf), bw=float(bw), tint=float(tint), mjd=mjd, timetype=timetype)


class Observation(object):
    """What ``empty_eht_obs`` returns -- ``array``, ``times`` (nt,) hours, ``gmst`` (nt,) hours, ``pairs`` (nvis, 2), ``uv``
    (nt, nvis, 2) float64 wavelengths, ``up`` (nt, nvis) bool, ``sigma`` (nt, nvis) Jy, ``elevation`` (nt, nsites) radians and the
    scalars ``ra`` (hours), ``dec`` (degrees), ``rf``, ``bw``, ``tint`` -- and the way from complex visibilities to the targets,
    sigmas and closure tables the operators of this module take (``data``).  Every baseline is kept in every frame; one that is
    not ``up`` carries no weight.  Parity with ehtim's scan bookkeeping is not pinned (``empty_eht_obs``)."""

    def __init__(self, array, times, gmst, pairs, uv, up, sigma, elevation, ra, dec, rf, bw, tint, mjd=None, timetype='GMST'):
        self.array, self.times, self.gmst, self.pairs = array, times, gmst, pairs
        self.uv = np.ascontiguousarray(uv, dtype=np.float64)
        self.up, self.sigma, self.elevation = np.asarray(up, dtype=bool), np.asarray(sigma, dtype=np.float64), elevation
        self.ra, self.dec, self.rf, self.bw, self.tint, self.mjd, self.timetype = ra, dec, rf, bw, tint, mjd, timetype
        self._min_quads = {}                                   # up stations -> the independent quadrangles of count='min'

    @property
    def nt(self):
        return int(self.uv.shape[0])

    @property
    def nvis(self):
        return int(self.uv.shape[1])

    def dft(self, fov, npix):
        """The ``DirectDFT`` of ``uv`` for images of ``npix`` pixels over ``fov`` radians."""
        return DirectDFT(self.uv, fov, npix)

    def pol_dft(self, fov, npix, weights=None):
        """The ``PolDFT`` of ``uv`` for images of ``npix`` pixels over ``fov`` radians."""
        return PolDFT(self.uv, fov, npix, weights=weights)

    def _per_baseline(self, vis, what):
        """``what`` (nt, nvis) shaped to broadcast against vis (nt, [S,] nvis)."""
        if vis.ndim not in (2, 3) or vis.shape[0] != self.nt or vis.shape[-1] != self.nvis:
            raise AttributeError('vis should have the shape ({}, [S,] {}), got {}'.format(self.nt, self.nvis, vis.shape))
        return what if vis.ndim == 2 else what[:, None, :]

    def add_thermal_noise(self, vis, seed=None):
        """vis (nt, [S,] nvis) plus complex Gaussian noise of ``sigma`` per real and imaginary part, 0 where the baseline is not
        up; complex64.  One call ``np.random.default_rng(seed).standard_normal(vis.shape + (2,))``: [..., 0] the real parts,
        [..., 1] the imaginary ones.  A host function."""
        vis = np.asarray(vis)
        sigma, up = self._per_baseline(vis, self.sigma), self._per_baseline(vis, self.up)
        n = np.random.default_rng(seed).standard_normal(vis.shape + (2,))
        noisy = vis.astype(np.complex128) + sigma * (n[..., 0] + 1j * n[..., 1])
        return np.where(up, noisy, 0.0).astype(np.complex64)

    def apply_gains(self, vis, gains):
        """vis[f, [s,] k] G[f, a_k] conj(G[f, b_k]) with (a_k, b_k) = ``pairs[k]``: complex station gains ``gains`` (nt, nsites)
        (``station_gains``) on visibilities (nt, [S,] nvis), the same on every Stokes plane; complex128.  A host function."""
        vis = np.asarray(vis).astype(np.complex128)
        gains = np.asarray(gains, dtype=np.complex128)
        if gains.shape != (self.nt, len(self.array)):
            raise AttributeError('gains should have the shape ({}, {}), got {}'.format(self.nt, len(self.array), gains.shape))
        factor = gains[:, self.pairs[:, 0]] * np.conj(gains[:, self.pairs[:, 1]])
        return vis * self._per_baseline(vis, factor)

    # -- closure sets
    def _stations_up(self, f):
        return tuple(sorted(set(self.pairs[self.up[f]].ravel().tolist())))

    def _frame_triangles(self, stations, count):
        if count == 'max':
            return [(a, b, c) for i, a in enumerate(stations) for j, b in enumerate(stations[i + 1:], i + 1) for c in stations[j + 1:]]
        ref = min(stations, key=lambda s: (self.array.sefd[s], s))          # lowest SEFD, ties by lowest index
        rest = [s for s in stations if s != ref]
        return [tuple(sorted((ref, a, b))) for i, a in enumerate(rest) for b in rest[i + 1:]]

    def _frame_quadrangles(self, stations, count):
        m = len(stations)
        if m < 4:
            return []
        st = np.asarray(stations)
        cand = [tuple(map(tuple, q)) for q in st[closure_quadrangles(m)].tolist()]
        if count == 'max':
            return cand
        if stations not in self._min_quads:
            # a greedy pass over the candidates keeps each one that raises the rank of the +-1 design matrix over the baselines,
            # until the m (m - 3) / 2 independent log closure amplitudes are found.  `basis` is kept in reduced row echelon form.
            col = {p: i for i, p in enumerate((a, b) for i, a in enumerate(stations) for b in stations[i + 1:])}
            need, keep = m * (m - 3) // 2, []
            basis, pivots = np.zeros((need, len(col))), []
            for q in cand:
                row = np.zeros(len(col))
                for leg, p in enumerate(q):
                    row[col[p]] += 1.0 if leg < 2 else -1.0
                r = len(keep)
                row -= row[pivots] @ basis[:r]
                p = int(np.argmax(np.abs(row)))
                if abs(row[p]) < 1e-9:
                    continue
                row /= row[p]
                basis[:r] -= np.outer(basis[:r, p], row)
                basis[r] = row
                pivots.append(p)
                keep.append(q)
                if len(keep) == need:
                    break
            self._min_quads[stations] = keep
        return self._min_quads[stations]

    def closure_sets(self, count='min', triangles=True, quadrangles=True):
        """The global closure tables of all frames and who is observed when: (triangles, tri_obs, quadrangles, quad_obs) --
        station triples (a < b < c), (nt, ntri) bool, quadrangles of station pairs in the form of ``closure_quadrangles`` and
        (nt, nquad) bool; the tables are the sorted union of the frames' sets (None, None where not asked for).

        count='max': per frame every triangle whose three baselines are up and both forms of every quadruple whose baselines are
        up.  count='min': per frame an independent set -- the (m - 1)(m - 2) / 2 triangles through the up station of lowest SEFD
        (ties: lowest index) and m (m - 3) / 2 quadrangles of full rank picked from the same two forms in a fixed order."""
        if count not in ('min', 'max'):
            raise AttributeError("count ({}) should be 'min' or 'max'".format(count))
        index = {tuple(p): i for i, p in enumerate(self.pairs.tolist())}
        stations = [self._stations_up(f) for f in range(self.nt)]
        tri_legs = lambda t: ((t[0], t[1]), (t[1], t[2]), (t[0], t[2]))
        out = []
        for want, per_frame, legs in ((triangles, self._frame_triangles, tri_legs), (quadrangles, self._frame_quadrangles, lambda q: q)):
            if not want:
                out += [None, None]
                continue
            of_stations = {st: per_frame(st, count) if st else [] for st in set(stations)}
            sets = [{t for t in of_stations[st] if all(self.up[f, index[p]] for p in legs(t))} for f, st in enumerate(stations)]
            table = sorted(set().union(*sets))
            out += [table, np.array([[t in s for t in table] for s in sets], dtype=bool).reshape(self.nt, len(table))]
        return tuple(out)

    def data(self, vis, dtype, count='min', debias=True):
        """Targets, sigmas and closure tables of complex visibilities ``vis`` (nt, [S,] nvis) as the operators take them: a dict
        term -> (target, sigma) for every term of ``dtype`` ('vis', or 'amp', 'cphase', 'logcamp' and their '+'-joined sets in
        that order), plus 'triangles' and 'quadrangles' (station tuples, one table for all frames; None when no term needs it).

        'vis': (vis, sigma).  'amp': sqrt(max(|V|^2 - sigma^2, 0)) with ``debias`` else |V|, sigma.  'cphase': the closure phase
        of vis (radians, ``ClosureDFT.closure_phases``) with sqrt(sum_legs (sigma_l / |V_l|)^2).  'logcamp':
        ``ClosureDFT.log_closure_amplitudes`` of the amplitudes (debiased with ``debias``) with sqrt(sum_legs (sigma_l / |V_l|)^2)
        over the four legs, |V_l| the same amplitudes.  ``count``: the closure sets (``closure_sets``).

        A baseline, triangle or quadrangle that a frame does not observe -- and one with a leg of zero amplitude -- gets the
        target 0 and the sigma +inf: every term of the losses divides by sigma, so it adds exactly 0 to the loss and to the
        gradient.  AttributeError when no frame observes a triangle / quadrangle that ``dtype`` needs.

        The polarimetric terms 'pvis', 'm' and 'pvis+m' take ``vis`` (nt, S >= 3, nvis) of the planes I, Q, U[, V] and give one
        complex128 target and one sigma (nt, nvis) per term (``PolDFT``).  'pvis': Q~ + i U~ with sqrt(2) sigma.  'm': P / I~ with
        sigma sqrt(2 + |m|^2) / |I~|, |I~| debiased with ``debias`` -- first-order propagation of equal thermal noise on the three
        planes.  An unobserved baseline and one with I~ == 0 (or debiased to 0) get the target 0 and the sigma +inf.  The two
        families do not mix in one dtype: 'cphase+m' is an AttributeError; add the steps (``TrainStep.__add__``)."""
        terms = tuple(str(dtype).split('+'))
        if any(t in POL_TERMS for t in terms):
            return self._pol_data(vis, terms, dtype, debias)
        if terms != ('vis',) and (terms != tuple(t for t in CLOSURE_TERMS if t in terms) or len(set(terms)) != len(terms)):
            raise AttributeError("dtype ({}) should be 'vis' or a '+'-joined set of {} in that order".format(dtype, CLOSURE_TERMS))
        vis = np.asarray(vis).astype(np.complex128)
        up, sigma = self._per_baseline(vis, self.up), self._per_baseline(vis, self.sigma)
        up, sigma = np.broadcast_to(up, vis.shape), np.broadcast_to(sigma, vis.shape)
        out = {'triangles': None, 'quadrangles': None}
        s_base = np.where(up, sigma, np.inf)
        amp = np.abs(vis)
        amp_db = np.sqrt(np.maximum(amp ** 2 - sigma ** 2, 0.0)) if debias else amp
        if 'vis' in terms:
            out['vis'] = (np.where(up, vis, 0.0).astype(np.complex64), s_base)
        if 'amp' in terms:
            out['amp'] = (np.where(up, amp_db, 0.0), s_base)
        if 'cphase' in terms or 'logcamp' in terms:
            tris, tri_obs, quads, quad_obs = self.closure_sets(count, 'cphase' in terms, 'logcamp' in terms)
            for name, table in (('cphase', tris), ('logcamp', quads)):
                if name in terms and not table:
                    raise AttributeError("dtype='{}': no frame observes a {}".format(name, 'triangle' if name == 'cphase' else 'quadrangle'))
            op = ClosureDFT(self.uv, 1.0, 1, pairs=self.pairs, triangles=tris, quadrangles=quads)       # (only its tables are used)
            shaped = lambda obs: obs if vis.ndim == 2 else obs[:, None, :]
            with np.errstate(divide='ignore', invalid='ignore'):
                if 'cphase' in terms:
                    snr2 = (sigma / amp) ** 2
                    sig = np.sqrt(sum(snr2[..., op.tri[:, leg]] for leg in range(3)))
                    ok = shaped(tri_obs) & np.isfinite(sig)
                    out['cphase'] = (np.where(ok, op.closure_phases(vis), 0.0), np.where(ok, sig, np.inf))
                    out['triangles'] = tris
                if 'logcamp' in terms:
                    snr2 = (sigma / amp_db) ** 2
                    sig = np.sqrt(sum(snr2[..., op.quad[:, leg]] for leg in range(4)))
                    ok = shaped(quad_obs) & np.isfinite(sig)
                    out['logcamp'] = (np.where(ok, op.log_closure_amplitudes(amp_db), 0.0), np.where(ok, sig, np.inf))
                    out['quadrangles'] = quads
        return out


    def _pol_data(self, vis, terms, dtype, debias):
        if terms != tuple(t for t in POL_TERMS if t in terms) or len(set(terms)) != len(terms):
            if all(t in POL_TERMS + CLOSURE_TERMS + ('vis',) for t in terms) and not all(t in POL_TERMS for t in terms):
                raise AttributeError("dtype ({}) mixes the polarimetric terms {} with another family: build one step per family and add "
                                     "them (TrainStep.__add__)".format(dtype, POL_TERMS))
            raise AttributeError("dtype ({}) should be a '+'-joined set of {} in that order".format(dtype, POL_TERMS))
        vis = np.asarray(vis).astype(np.complex128)
        if vis.ndim != 3 or vis.shape[1] < 3:
            raise AttributeError("dtype='{}' needs vis (nt, S >= 3, nvis) of the planes I, Q, U; got {}".format(dtype, vis.shape))
        self._per_baseline(vis, self.up)
        out = {'triangles': None, 'quadrangles': None}
        vI, P = vis[:, 0], vis[:, 1] + 1j * vis[:, 2]
        if 'pvis' in terms:
            out['pvis'] = (np.where(self.up, P, 0.0), np.where(self.up, np.sqrt(2.0) * self.sigma, np.inf))
        if 'm' in terms:
            amp = np.abs(vI)
            amp_db = np.sqrt(np.maximum(amp ** 2 - self.sigma ** 2, 0.0)) if debias else amp
            ok = self.up & (amp > 0) & (amp_db > 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                m = np.where(ok, P / np.where(ok, vI, 1.0), 0.0)
                sig = self.sigma * np.sqrt(2.0 + np.abs(m) ** 2) / amp_db
            out['m'] = (m, np.where(ok, sig, np.inf))
        return out


def station_gains(obs, amp_sigma=0.1, phase_sigma=np.pi, seed=None):
    """Random complex station gains (nt, nsites) complex128 for ``Observation.apply_gains`` / ``observe_same``:
    (1 + amp_sigma n_1) exp(i phase_sigma n_2) per frame and station, from one call
    ``np.random.default_rng(seed).standard_normal((nt, nsites, 2))``: [..., 0] is n_1, [..., 1] is n_2.  The default phase_sigma
    leaves no phase information.  A host function; the numbers stand for no particular site."""
    n = np.random.default_rng(seed).standard_normal((obs.nt, len(obs.array), 2))
    return (1.0 + float(amp_sigma) * n[..., 0]) * np.exp(1j * float(phase_sigma) * n[..., 1])


def observe_host(vis, obs, thermal_noise=True, seed=None, gains=None):
    """The host part of ``observe_same``: clean visibilities ``vis`` (nt, [S,] nvis) -> station ``gains`` (None: none), then
    thermal noise, 0 where the baseline is not up; complex64 NumPy."""
    if gains is not None:
        vis = obs.apply_gains(vis, gains)
    if thermal_noise:
        return obs.add_thermal_noise(vis, seed)
    return np.where(obs._per_baseline(vis, obs.up), vis, 0.0).astype(np.complex64)


def observe_same(movie, obs, fov, thermal_noise=True, seed=None, device=None, gains=None):
    """Synthetic visibilities of ``movie`` (nt, [S,] H, W), one frame per scan of ``obs`` (an ``Observation``), over ``fov`` radians:
    the clean visibilities from ``DirectDFT.observe`` on the device (``HipError`` without one), plus ``obs.add_thermal_noise`` with
    ``thermal_noise``; 0 where the baseline is not up.  Returns complex64 NumPy (nt, [S,] nvis).  ``gains`` (nt, nsites) complex
    (``station_gains``) multiply the clean visibilities before the thermal noise, V[f, s, k] G[f, a_k] conj(G[f, b_k]), the same on
    every Stokes plane (``Observation.apply_gains``).  The closure terms on Stokes I and the fractional polarisation 'm'
    (``PolDFT``) do not see such gains; 'vis', 'amp' and 'pvis' do.  The reference hands the movie to ehtim, which also corrupts
    with D-terms and with gains that differ between the two polarisations: those are out of scope here."""
    movie = np.asarray(movie) if not hasattr(movie, 'detach') else movie
    vis = obs.dft(fov, tuple(movie.shape[-2:])).observe(movie, device=device).cpu().numpy()
    return observe_host(vis, obs, thermal_noise, seed, gains)
