"""Kerr null geodesics for the image plane: an own ray tracer in place of the external ``kgeo`` package.

The reference's ``bhnerf.kgeo.image_plane_geos`` (``kgeo.py:6-63``) wraps ``kgeo.raytrace_ana`` of an external,
un-vendored package and returns an ``xarray.Dataset``.  Neither is available here, so this module integrates the
geodesics itself and returns a ``Geodesics`` record (attribute access to NumPy arrays with the same names and the
same ``(alpha, beta, geo)`` layout).  **Parity unpinned** against the external tracer; what is checked instead
(``tests/test_geodesics_cpu.py``): the constants of motion along every ray (``(dr/dλ)² = R(r)``, ``(dθ/dλ)² = Θ(θ)``),
straight lines and Euclidean light-travel time for ``M → 0``, the Schwarzschild shadow radius ``√27 M`` and the
equatorial reflection symmetry.

Method (Boyer-Lindquist coordinates, ``G = c = 1``, photon energy at infinity ``E``): in Mino time ``λ``
(``d(affine) = Σ dλ``) the radial and polar motions separate,

    (dr/dλ)² = R(r) = (r² + a² − a ℓ)² − Δ (η + (ℓ − a)²),      (dθ/dλ)² = Θ(θ) = η + a² cos²θ − ℓ² cot²θ,
    dφ/dλ = a (r² + a² − a ℓ)/Δ − a + ℓ / sin²θ,               dt/dλ = (r² + a²)(r² + a² − a ℓ)/Δ + a (ℓ − a sin²θ),

with ``ℓ = −α sin i`` and ``η = (α² − a²) cos² i + β²`` for the image-plane coordinates ``(α, β)`` of an observer at
inclination ``i`` (Bardeen 1973).  The second-order form ``r'' = R'(r)/2``, ``θ'' = Θ'(θ)/2`` is integrated backwards
from the observer with classical RK4 — no sign bookkeeping at the turning points; away from them the radial
velocity is re-derived from ``R(r)`` after every step — with a per-ray step
``dλ = h (1 + r/r_c) / r²`` (radial steps of ≈ h(1 + r/r_c): a few hundredths of M near the hole, geometric far away), until the ray falls
through the horizon or is back at the observer's radius (finished rays are compacted away).  A second pass with the
now known total Mino time of every ray writes its ``ngeo`` samples, uniform in Mino time, as the steps cross them, which is where ``dtau`` (the Mino step) of the radiative-transfer integrand ``g² · dtau · Σ`` comes from.

``equatorial_crossings`` runs the same stepping in one pass and returns where every ray meets the plane ``θ = π/2`` for the first,
second, … time: the crossing is located inside its RK4 step on the step's cubic Hermite interpolant (the one the samples are written
with).  It is the primitive of ``emission.equatorial_ring`` and ``kgeo.equatorial_lensing``; ``ray_geos`` is ``image_plane_geos`` for a
list of rays.
"""
import numpy as np


class Geodesics(dict):
    """Mapping with attribute access: the fields of the reference's geodesic dataset as NumPy arrays."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__

    @property
    def dims(self):
        shape = self['r'].shape
        if len(shape) == 2:                              # the ray-list form (ray_geos)
            return {'pix': shape[0], 'geo': shape[1]}
        return {'alpha': shape[0], 'beta': shape[1], 'geo': shape[2]}

    def fillna(self, value):
        """Copy with the NaNs of every floating array replaced (``xarray.Dataset.fillna``, used by alma.py:43)."""
        out = Geodesics()
        for k, v in self.items():
            arr = np.asarray(v)
            out[k] = np.where(np.isnan(arr), value, arr) if arr.dtype.kind == 'f' and arr.ndim else v
        return out


class DeviceGeodesics(Geodesics):
    """The record of ``image_plane_geos(..., backend='hip', resident=True)``: the keys and shapes of ``Geodesics``, every array field a
    float64 torch tensor on one device (created there by ``bhn_rec_build``, include/bhnerf_rec.h), the scalars floats.
    ``kgeo.emission_factors`` and ``network.raytracing_args`` read it where it is; ``numpy()`` gives the ordinary record."""

    @property
    def device(self):
        return self['r'].device

    def fillna(self, value):
        """Copy with the NaNs (and nothing else) of every floating tensor replaced, on the device."""
        import torch
        out = DeviceGeodesics()
        for k, v in self.items():
            if isinstance(v, torch.Tensor) and v.is_floating_point() and v.ndim:
                out[k] = torch.where(torch.isnan(v), torch.as_tensor(value, dtype=v.dtype, device=v.device), v)
            else:
                out[k] = v
        return out

    def numpy(self):
        """The ``Geodesics`` record of NumPy arrays with the same contents."""
        import torch
        return Geodesics((k, v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in self.items())


def kerr_functions(r, theta, spin, M=1.0):
    """Δ, Σ, Ξ and the frame-dragging frequency ω of the Kerr metric (spin in units of M)."""
    a = spin * M
    Delta = r ** 2 - 2.0 * M * r + a ** 2
    Sigma = r ** 2 + a ** 2 * np.cos(theta) ** 2
    Xi = (r ** 2 + a ** 2) ** 2 - Delta * a ** 2 * np.sin(theta) ** 2
    omega = 2.0 * a * M * r / Xi
    return Delta, Sigma, Xi, omega


def radial_potential(r, a, lam, eta, M=1.0):
    Delta = r ** 2 - 2.0 * M * r + a ** 2
    return (r ** 2 + a ** 2 - a * lam) ** 2 - Delta * (eta + (lam - a) ** 2)


def angular_potential(theta, a, lam, eta):
    return eta + a ** 2 * np.cos(theta) ** 2 - lam ** 2 / np.tan(theta) ** 2


def _rhs(y, a, lam, eta, M):
    r, th, vr, vth = y[0], y[1], y[4], y[5]
    s, c = np.sin(th), np.cos(th)
    Delta = r ** 2 - 2.0 * M * r + a ** 2
    P = r ** 2 + a ** 2 - a * lam
    # R'(r)/2 and Θ'(θ)/2
    ar = 2.0 * r * P - (r - M) * (eta + (lam - a) ** 2)
    ath = -a ** 2 * s * c + lam ** 2 * c / s ** 3
    dph = a * P / Delta - a + lam / s ** 2
    dt = (r ** 2 + a ** 2) * P / Delta + a * (lam - a * s ** 2)
    return np.stack([vr, vth, dph, dt, ar, ath])


def _initial_state(alpha, beta, a, inc, distance, M):
    lam = -alpha * np.sin(inc)
    eta = (alpha ** 2 - a ** 2) * np.cos(inc) ** 2 + beta ** 2
    r0 = np.full_like(alpha, float(distance))
    th0 = np.full_like(alpha, inc)
    vr0 = -np.sqrt(np.clip(radial_potential(r0, a, lam, eta, M), 0.0, None))            # inwards, back in time
    vth0 = -np.sign(beta) * np.sqrt(np.clip(angular_potential(th0, a, lam, eta), 0.0, None))
    return np.stack([r0, th0, np.zeros_like(r0), np.zeros_like(r0), vr0, vth0]), lam, eta


def _rk4_step(y, a, lm, et, M, h, r_c):
    """One RK4 step of every ray in ``y`` (6, m): ``(dl, k1, y_new)``, the step lengths, the right-hand side at ``y`` and the
    states after the step.  Whether a ray takes its step is the caller's rule (``_integrate``, ``_integrate_crossings``)."""
    # (the centrifugal term of Theta is stiff next to the poles: up to 20x smaller steps there)
    dl = h * (1.0 + y[0] / r_c) / y[0] ** 2 * np.clip((np.sin(y[1]) / 0.25) ** 2, 0.05, 1.0)
    k1 = _rhs(y, a, lm, et, M)
    k2 = _rhs(y + 0.5 * dl * k1, a, lm, et, M)
    k3 = _rhs(y + 0.5 * dl * k2, a, lm, et, M)
    k4 = _rhs(y + dl * k3, a, lm, et, M)
    y_new = y + dl / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    # keep the first integrals (dr/dlambda)^2 = R(r), (dtheta/dlambda)^2 = Theta(theta): far from the hole dr/dlambda ~ r^2 ~
    # 1e6 and a relative RK4 error of 1e-10 there is an absolute error of 1e2 in (dr/dlambda)^2 at the turning point; away
    # from turning points the velocities are therefore re-derived from the potentials (sign kept), near them the
    # second-order form runs free
    Rn = radial_potential(y_new[0], a, lm, et, M)
    y_new[4] = np.where(Rn > 1e-2 * y_new[0] ** 4, np.sign(y_new[4]) * np.sqrt(np.abs(Rn)), y_new[4])
    Tn = angular_potential(y_new[1], a, lm, et)
    y_new[5] = np.where(Tn > 1e-2 * (et + a * a + lm ** 2), np.sign(y_new[5]) * np.sqrt(np.abs(Tn)), y_new[5])
    return dl, k1, y_new


def _hermite(w, dl, y, k1, y_new, f_new):
    """Cubic Hermite combination of the two ends of a step at ``w`` of it (values and derivatives at both ends)."""
    w2, w3 = w * w, w * w * w
    return (2 * w3 - 3 * w2 + 1) * y + (w3 - 2 * w2 + w) * dl * k1 + (3 * w2 - 2 * w3) * y_new + (w3 - w2) * dl * f_new


def _integrate(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, targets=None):
    """RK4 over all rays with the finished ones compacted away.  Without ``targets``: returns each ray's final Mino
    time and state.  With ``targets`` (n, ngeo) increasing Mino times: returns the states interpolated at them,
    shape (7, n, ngeo) with rows (mino, r, theta, phi, t, vr, vth)."""
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    beta = np.asarray(beta, dtype=np.float64).ravel()
    a = float(spin) * M
    inc = float(inclination)
    if not (0.0 < inc <= 0.5 * np.pi + 1e-12):
        raise ValueError('inclination must be in (0, pi/2]')
    n = alpha.size
    y, lam, eta = _initial_state(alpha, beta, a, inc, distance, M)
    r_hor = M + np.sqrt(max(M * M - a * a, 0.0))
    idx = np.arange(n)                                   # rays still being integrated (compacted)
    mino = np.zeros(n)
    end_mino, end_y = np.zeros(n), y.copy()
    out = nxt = None
    if targets is not None:
        ngeo = targets.shape[1]
        out = np.zeros((7, n, ngeo))
        nxt = np.zeros(n, dtype=np.int64)                # next sample of every ray (global indexing)
    for step in range(1, max_steps + 1):
        lm, et = lam[idx], eta[idx]
        dl, k1, y_new = _rk4_step(y, a, lm, et, M, h, r_c)
        captured = ~(y_new[0] > r_hor * 1.02)              # (also catches a NaN): the step is not taken, the ray ends here
        mino_new = mino + dl
        if targets is not None:                            # samples crossed by this step: cubic Hermite in Mino time
            ok = ~captured                                 # (value and derivative at both ends of the step: O(h^4) like
            f_new = None                                   #  the RK4 step itself; linear interpolation left O(h^2))
            while True:
                g_idx = idx
                k = np.minimum(nxt[g_idx], ngeo - 1)
                tgt = targets[g_idx, k]
                hit = ok & (nxt[g_idx] < ngeo) & (tgt <= mino_new)
                if not hit.any():
                    break
                w = ((tgt - mino) / np.where(dl > 0, dl, 1.0))[hit]
                rows = g_idx[hit]
                if f_new is None:
                    f_new = _rhs(y_new, a, lm, et, M)
                out[0, rows, k[hit]] = tgt[hit]
                out[1:, rows, k[hit]] = _hermite(w, dl[hit], y[:, hit], k1[:, hit], y_new[:, hit], f_new[:, hit])
                nxt[rows] += 1
        y = np.where(captured, y, y_new)
        mino = np.where(captured, mino, mino_new)
        done = captured | ((y[0] > distance) & (y[4] > 0.0))
        if done.any():
            rows = idx[done]
            end_mino[rows], end_y[:, rows] = mino[done], y[:, done]
            keep = ~done
            idx, y, mino = idx[keep], y[:, keep], mino[keep]
            if idx.size == 0:
                break
    else:
        raise RuntimeError('geodesic integration did not terminate in %d steps' % max_steps)
    if targets is None:
        return end_mino, end_y, lam, eta
    # rounding can leave the very last sample (target = end of the ray) unwritten: it is the end state
    miss = nxt < ngeo
    for j in np.nonzero(miss)[0]:
        out[0, j, nxt[j]:] = end_mino[j]
        out[1:, j, nxt[j]:] = end_y[:, j, None]
    return out, lam, eta


HALF_PI = 0.5 * np.pi
ROOT_BISECTIONS = 64             # EQ_BISECTIONS of csrc/equatorial.h
PLANE_MARGIN = 1e-6              # an observer this close to the equatorial plane is refused


def _check_off_plane(inc):
    if not (0.0 < inc <= 0.5 * np.pi + 1e-12):
        raise ValueError('inclination must be in (0, pi/2]')
    if not (abs(inc - HALF_PI) > PLANE_MARGIN):
        raise ValueError('inclination must be away from pi/2: the observer sits in the plane')


def _hermite_root(below, dl, th, f, thn, fn):
    """Where in (0, 1] of a step the cubic Hermite interpolant of theta leaves the side of the equatorial plane it starts on
    (``below``: theta < pi/2 at the step's start).  Bisection on [0, 1], always all ROOT_BISECTIONS halvings: after 53 the two ends
    are neighbouring doubles, the rest change nothing; the upper end is returned.  ``eq_hermite_root`` of csrc/equatorial.h is this
    function operation for operation."""
    lo, hi = np.zeros_like(dl), np.ones_like(dl)
    for _ in range(ROOT_BISECTIONS):
        mid = 0.5 * (lo + hi)
        g = _hermite(mid, dl, th, f, thn, fn) - HALF_PI
        same = np.where(below, g < 0.0, g > 0.0)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return hi


def _integrate_crossings(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, nmax):
    """The first ``nmax`` meetings of every ray with the equatorial plane: ``(cross (7, n, nmax), count (n), lam, eta)``, rows
    (mino, r, theta, phi, t, vr, vth) of the forward equations, NaN in the columns a ray does not reach.  The stepping of
    ``_integrate`` in one pass; a taken step with theta - pi/2 of opposite sign at its ends, or with its new end exactly on pi/2,
    holds one crossing, at the root of the step's cubic Hermite interpolant of theta, and the rows are that interpolant there.  A
    ray is dropped at its end or after its ``nmax``-th crossing."""
    alpha = np.asarray(alpha, dtype=np.float64).ravel()
    beta = np.asarray(beta, dtype=np.float64).ravel()
    a = float(spin) * M
    inc, nmax = float(inclination), int(nmax)
    _check_off_plane(inc)
    if nmax < 1:
        raise ValueError('nmax must be at least 1')
    n = alpha.size
    y, lam, eta = _initial_state(alpha, beta, a, inc, distance, M)
    r_hor = M + np.sqrt(max(M * M - a * a, 0.0))
    idx = np.arange(n)
    mino = np.zeros(n)
    cross = np.full((7, n, nmax), np.nan)
    count = np.zeros(n, dtype=np.int32)
    for step in range(1, max_steps + 1):
        lm, et = lam[idx], eta[idx]
        dl, k1, y_new = _rk4_step(y, a, lm, et, M, h, r_c)
        captured = ~(y_new[0] > r_hor * 1.02)
        d0, d1 = y[1] - HALF_PI, y_new[1] - HALF_PI
        hit = ~captured & (((d0 < 0.0) & (d1 > 0.0)) | ((d0 > 0.0) & (d1 < 0.0)) | (d1 == 0.0))
        if hit.any():
            yh, kh, nh, dh = y[:, hit], k1[:, hit], y_new[:, hit], dl[hit]
            fh = _rhs(nh, a, lm[hit], et[hit], M)
            w = _hermite_root(d0[hit] < 0.0, dh, yh[1], kh[1], nh[1], fh[1])
            rows = idx[hit]
            cross[0, rows, count[rows]] = mino[hit] + w * dh
            cross[1:, rows, count[rows]] = _hermite(w, dh, yh, kh, nh, fh)
            count[rows] += 1
        y = np.where(captured, y, y_new)
        mino = np.where(captured, mino, mino + dl)
        done = captured | ((y[0] > distance) & (y[4] > 0.0)) | (count[idx] >= nmax)
        if done.any():
            keep = ~done
            idx, y, mino = idx[keep], y[:, keep], mino[keep]
            if idx.size == 0:
                break
    else:
        raise RuntimeError('geodesic integration did not terminate in %d steps' % max_steps)
    return cross, count, lam, eta


BACKENDS = ('numpy', 'hip')
SAMPLE_ROWS = ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth')


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError('backend must be one of %s, not %r' % (', '.join(repr(b) for b in BACKENDS), backend))


def _trace_device(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, ngeo, device=None):
    """``bhn_kerr_trace`` (include/bhnerf_kerr.h; csrc/kerr_trace.hip restates ``_integrate`` with one GPU lane per ray) on
    one set of rays: ``(end (7, n), samples (7, n, ngeo) or None, lam, eta, dev)``, ``end`` and ``samples`` float64 tensors on the torch
    device ``dev``, ``lam`` and ``eta`` NumPy arrays.  Raises ``_integrate``'s RuntimeError when a ray is not finished after
    ``max_steps``."""
    import torch
    from . import _hip
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).ravel()
    beta = np.ascontiguousarray(beta, dtype=np.float64).ravel()
    inc = float(inclination)
    if not (0.0 < inc <= 0.5 * np.pi + 1e-12):
        raise ValueError('inclination must be in (0, pi/2]')
    lib = _hip.kerr_lib()
    if not torch.cuda.is_available():
        raise _hip.HipError("backend='hip' needs a HIP device (there is no CPU fallback; backend='numpy' is the host tracer)")
    dev = torch.device('cuda' if device is None else device)
    n, ngeo = alpha.size, int(ngeo)
    _, lam, eta = _initial_state(alpha, beta, float(spin) * M, inc, distance, M)
    with torch.cuda.device(dev):
        a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
        end = torch.empty((7, n), dtype=torch.float64, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        samples = torch.empty((7, n, ngeo), dtype=torch.float64, device=dev) if ngeo > 0 else None
        _hip.kerr_check(lib.bhn_kerr_trace(_hip.ptr(a_d), _hip.ptr(b_d), n, float(spin), inc, float(distance), float(M), float(h), float(r_c),
                                      int(max_steps), ngeo, _hip.ptr(samples), _hip.ptr(end), _hip.ptr(status), _hip.stream_ptr(dev)))
        if bool((status < 0).any()):
            raise RuntimeError('geodesic integration did not terminate in %d steps' % max_steps)
        return end, samples, lam, eta, dev


def _trace_hip(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, ngeo, device=None):
    """``_trace_device`` with its results downloaded: ``(end (7, n), samples (7, n, ngeo) or None, lam, eta)`` as NumPy arrays, ``end``
    rows final Mino time, r, theta, phi, t, vr, vth."""
    end, samples, lam, eta, _ = _trace_device(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, ngeo, device)
    return end.cpu().numpy(), (samples.cpu().numpy() if samples is not None else None), lam, eta


def trace(alpha, beta, spin, inclination, distance=1000.0, M=1.0, h=0.02, r_c=5.0, max_steps=400000, backend='numpy', device=None):
    """Integrate one geodesic per (alpha, beta) backwards from the observer until it is captured or has escaped.
    Returns ``(mino_end, state_end, lam, eta)`` with ``state_end`` rows ``(r, theta, phi, t, vr, vth)`` (phi and t of
    the forward equations: negate them for the backward ray).  ``backend='hip'`` runs the same integration on the GPU
    (``device``: a torch device, default the current one)."""
    _check_backend(backend)
    if backend == 'hip':
        end, _, lam, eta = _trace_hip(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, 0, device)
        return end[0], end[1:], lam, eta
    return _integrate(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps)


def _crossings_hip(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, nmax, device=None):
    """``bhn_eql_crossings`` (include/bhnerf_eql.h; csrc/equatorial.hip restates ``_integrate_crossings`` with one GPU lane per
    ray): ``(cross (7, n, nmax), count (n), lam, eta)`` as NumPy arrays.  Raises the tracer's RuntimeError when a ray is neither
    finished nor at its ``nmax``-th crossing after ``max_steps``."""
    import torch
    from . import _hip
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).ravel()
    beta = np.ascontiguousarray(beta, dtype=np.float64).ravel()
    inc, nmax = float(inclination), int(nmax)
    _check_off_plane(inc)
    if nmax < 1:
        raise ValueError('nmax must be at least 1')
    lib = _hip.eql_lib()
    if not torch.cuda.is_available():
        raise _hip.HipError("backend='hip' needs a HIP device (there is no CPU fallback; backend='numpy' is the host tracer)")
    dev = torch.device('cuda' if device is None else device)
    n = alpha.size
    _, lam, eta = _initial_state(alpha, beta, float(spin) * M, inc, distance, M)
    with torch.cuda.device(dev):
        a_d, b_d = torch.as_tensor(alpha, device=dev), torch.as_tensor(beta, device=dev)
        cross = torch.empty((7, n, nmax), dtype=torch.float64, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        _hip.eql_check(lib.bhn_eql_crossings(_hip.ptr(a_d), _hip.ptr(b_d), n, float(spin), inc, float(distance), float(M), float(h),
                                             float(r_c), int(max_steps), nmax, _hip.ptr(cross), _hip.ptr(count), _hip.ptr(status),
                                             _hip.stream_ptr(dev)))
        if bool((status < 0).any()):
            raise RuntimeError('geodesic integration did not terminate in %d steps' % max_steps)
        return cross.cpu().numpy(), count.cpu().numpy(), lam, eta


def equatorial_crossings(alpha, beta, spin, inclination, nmax=3, distance=1000.0, M=1.0, h=0.02, r_c=5.0, max_steps=400000,
                         backend='numpy', device=None):
    """Where the rays ``(alpha, beta)`` of the image-plane tracer meet the equatorial plane for the first, ..., ``nmax``-th time.

    Returns a ``Geodesics``-style record of arrays ``(n, nmax)``: ``mino, r, theta, phi, t, vr, vth`` at the crossings (column j: the
    (j+1)-th crossing counted from the observer, NaN where the ray has none), ``count`` (n) the crossings found, and the ray
    constants ``lam``, ``eta`` (n).  ``mino``, ``phi`` and ``t`` carry the sign convention of ``image_plane_geos``: negative along
    the ray.  The rays are followed exactly as ``trace`` follows them; a crossing is located inside its RK4 step on the step's cubic
    Hermite interpolant.  ``backend='hip'`` runs the same integration on the GPU (``bhn_eql_crossings``; ``device``: a torch device,
    default the current one).  The observer must not sit in the plane (inclination within 1e-6 of pi/2 is refused)."""
    _check_backend(backend)
    if backend == 'hip':
        cross, count, lam, eta = _crossings_hip(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, nmax, device)
    else:
        cross, count, lam, eta = _integrate_crossings(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, nmax)
    g = Geodesics(mino=-cross[0], r=cross[1], theta=cross[2], phi=-cross[3], t=-cross[4], vr=cross[5], vth=cross[6])
    g['count'], g['lam'], g['eta'] = count, lam, eta
    return g


def _sample_rays(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, ngeo, backend, device):
    """``ngeo`` samples per ray, uniform in Mino time: ``(samples (7, n, ngeo) with the rows SAMPLE_ROWS, lam, eta)``."""
    if backend == 'hip':
        _, samp, lam, eta = _trace_hip(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, ngeo, device)
        return samp, lam, eta
    mino_end, _, lam, eta = _integrate(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps)
    target = (np.arange(1, ngeo + 1)[None, :] / float(ngeo)) * mino_end[:, None]            # uniform in Mino time
    samp, _, _ = _integrate(alpha, beta, spin, inclination, distance, M, h, r_c, max_steps, targets=target)
    return samp, lam, eta


def _build_record(out, lam_all, eta_all, alpha, beta, spin, inclination, distance, E, M):
    """The ``Geodesics`` record of ``image_plane_geos`` / ``ray_geos`` from the sampled rows ``out`` (name -> (n, ngeo)) of n rays
    whose screen coordinates ``alpha``, ``beta`` have the shape the record's ray dimensions take."""
    ngeo = out['r'].shape[1]
    rays = alpha.shape
    shape3 = rays + (ngeo,)
    g = Geodesics()
    a = float(spin) * M
    r, th = out['r'].reshape(shape3), out['theta'].reshape(shape3)
    # the rays were followed backwards: coordinate time and azimuth run the other way
    g.update(r=r, theta=th, phi=-out['phi'].reshape(shape3), t=-out['t'].reshape(shape3), mino=-out['mino'].reshape(shape3))
    g['Delta'], g['Sigma'], g['Xi'], g['omega'] = kerr_functions(r, th, spin, M)
    g['x'] = r * np.sin(th) * np.cos(g['phi'])
    g['y'] = r * np.sin(th) * np.sin(g['phi'])
    g['z'] = r * np.cos(th)
    lam3, eta3 = lam_all.reshape(rays)[..., None], eta_all.reshape(rays)[..., None]
    g['R'] = radial_potential(r, a, lam3, eta3, M)
    g['Theta'] = angular_potential(th, a, lam3, eta3)
    g['vr'], g['vth'] = out['vr'].reshape(shape3), out['vth'].reshape(shape3)
    dtau = -g['mino'][..., :1] * np.ones(shape3)                                 # uniform Mino step of each ray (positive)
    g['dtau'] = dtau
    g['affine'] = -np.cumsum(g['Sigma'] * dtau, axis=-1)          # 0 at the observer, decreasing into the past: d(affine) = Σ dλ
    g['alpha'], g['beta'] = alpha, beta
    g['lam'], g['eta'] = lam_all.reshape(rays), eta_all.reshape(rays)
    g['spin'], g['inc'], g['M'], g['E'], g['r_o'] = float(spin), float(inclination), float(M), float(E), float(distance)
    return g


def _sampled_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, backend, device, verbose):
    """Trace the rays ``alpha``, ``beta`` (any common shape) ``chunk`` at a time and build their record."""
    n = alpha.size
    out = {k: np.empty((n, ngeo)) for k in SAMPLE_ROWS}
    lam_all, eta_all = np.empty(n), np.empty(n)
    af, bf = alpha.ravel(), beta.ravel()
    # beta = 0 exactly sits on the theta turning point of the observer: nudge it (measure-zero set of rays)
    bf = np.where(bf == 0.0, 1e-9, bf)
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(c0 + chunk, n))
        samp, lam, eta = _sample_rays(af[sl], bf[sl], spin, inclination, distance, M, h, 5.0, max_steps, ngeo, backend, device)
        lam_all[sl], eta_all[sl] = lam, eta
        for row, name in enumerate(SAMPLE_ROWS):
            out[name][sl] = samp[row]
        if verbose:
            print('traced rays %d-%d of %d' % (c0, sl.stop, n))
    return _build_record(out, lam_all, eta_all, alpha, beta, spin, inclination, distance, E, M)


def _check_resident(resident, backend):
    if resident and backend != 'hip':
        raise ValueError("resident=True keeps the record on the GPU: it needs backend='hip', not %r" % (backend,))


def _resident_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, device, verbose):
    """``_sampled_record`` without leaving the device: every chunk's samples go from ``bhn_kerr_trace`` straight into
    ``bhn_rec_build`` (include/bhnerf_rec.h), which writes the chunk's slab of the 18 per-point fields.  The host sends the screen
    coordinates and the rays' constants ``lam``, ``eta`` and reads the tracer's status.  Returns a ``DeviceGeodesics``."""
    import ctypes as C
    import torch
    from . import _hip
    n, ngeo = alpha.size, int(ngeo)
    if ngeo < 1:
        raise ValueError('ngeo must be at least 1')
    rays = alpha.shape
    af, bf = alpha.ravel(), beta.ravel()
    bf = np.where(bf == 0.0, 1e-9, bf)                    # (as in _sampled_record)
    lib = _hip.rec_lib()
    fields = dev = None
    lam_all, eta_all = np.empty(n), np.empty(n)
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(c0 + chunk, n))
        _, samples, lam, eta, dev = _trace_device(af[sl], bf[sl], spin, inclination, distance, M, h, 5.0, max_steps, ngeo, device)
        lam_all[sl], eta_all[sl] = lam, eta
        with torch.cuda.device(dev):
            if fields is None:
                fields = {k: torch.empty((n, ngeo), dtype=torch.float64, device=dev) for k in _hip.REC_FIELDS}
            lam_c, eta_c = torch.as_tensor(lam, device=dev), torch.as_tensor(eta, device=dev)
            out = _hip.bhn_rec_fields(*[fields[k][c0:].data_ptr() for k in _hip.REC_FIELDS])
            _hip.rec_check(lib.bhn_rec_build(_hip.ptr(samples), _hip.ptr(lam_c), _hip.ptr(eta_c), sl.stop - c0, ngeo, float(spin), float(M),
                                             C.byref(out), _hip.stream_ptr(dev)))
        if verbose:
            print('traced rays %d-%d of %d' % (c0, sl.stop, n))
    g = DeviceGeodesics()
    shape3 = rays + (ngeo,)
    g.update((k, fields[k].reshape(shape3)) for k in _hip.REC_FIELDS)              # the key order of _build_record
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev)
    g['alpha'], g['beta'] = up(alpha), up(beta)
    g['lam'], g['eta'] = up(lam_all.reshape(rays)), up(eta_all.reshape(rays))
    g['spin'], g['inc'], g['M'], g['E'], g['r_o'] = float(spin), float(inclination), float(M), float(E), float(distance)
    return g


def image_plane_geos(spin, inclination, alpha_range, beta_range, ngeo=100, num_alpha=64, num_beta=64, distance=1000.0,
                     E=1.0, M=1.0, randomize_subpixel_rays=False, verbose=False, h=0.02, chunk=65536, max_steps=400000,
                     backend='numpy', device=None, resident=False):
    """Kerr geodesics for the whole image plane (signature of ``bhnerf.kgeo.image_plane_geos``, kgeo.py:6-63).

    Returns a ``Geodesics`` record with arrays of shape ``(num_alpha, num_beta, ngeo)`` (per-ray constants
    ``(num_alpha, num_beta)``): ``r, theta, phi, t, x, y, z, mino, affine, dtau, Sigma, Delta, Xi, omega, R, Theta``,
    ``alpha, beta, lam, eta`` and the scalars ``spin, inc, M, E, r_o``.  ``t`` is the coordinate time relative to the
    arrival at the observer (negative along the ray), ``dtau`` the Mino step between consecutive samples.

    ``backend``: ``'numpy'`` (the default) integrates on the host, ``'hip'`` on the GPU (``bhn_kerr_trace``, one call per
    ``chunk`` rays on ``device``); the record is built from the samples by the same code either way.

    ``resident=True`` (``backend='hip'`` only) leaves the record where the tracer wrote its samples: ``bhn_rec_build`` builds the
    fields on the device and a ``DeviceGeodesics`` of float64 tensors comes back."""
    _check_backend(backend)
    _check_resident(resident, backend)
    alpha_1d = np.linspace(*alpha_range, num_alpha)
    beta_1d = np.linspace(*beta_range, num_beta)
    if randomize_subpixel_rays:
        alpha_1d = alpha_1d + (np.random.random(num_alpha) - 0.5) * (alpha_range[1] - alpha_range[0]) / max(num_alpha - 1, 1)
        beta_1d = beta_1d + (np.random.random(num_beta) - 0.5) * (beta_range[1] - beta_range[0]) / max(num_beta - 1, 1)
    alpha, beta = np.meshgrid(alpha_1d, beta_1d, indexing='ij')
    if resident:
        return _resident_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, device, verbose)
    return _sampled_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, backend, device, verbose)


def ray_geos(spin, inclination, alpha, beta, ngeo=100, distance=1000.0, E=1.0, M=1.0, verbose=False, h=0.02, chunk=65536,
             max_steps=400000, backend='numpy', device=None, resident=False):
    """The record of ``image_plane_geos`` for an arbitrary LIST of rays: ``alpha``, ``beta`` of n screen coordinates each; fields of
    shape ``(n, ngeo)``, per-ray constants ``(n,)``.  Stands in for ``kgeo.raytrace_ana(...).get_dataset()`` of the external
    package (dims ``(pix, geo)``), which the Gelles-2021 notebook of the reference calls; built by the same code as the grid form, so
    ``ray_geos`` on a grid's flattened rays holds the grid's record bit for bit.  ``resident=True``: as in ``image_plane_geos``."""
    _check_backend(backend)
    _check_resident(resident, backend)
    alpha = np.array(alpha, dtype=np.float64).ravel()
    beta = np.array(beta, dtype=np.float64).ravel()
    if alpha.shape != beta.shape or alpha.size < 1:
        raise ValueError('alpha and beta must be lists of the same length, at least one ray')
    if resident:
        return _resident_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, device, verbose)
    return _sampled_record(alpha, beta, spin, inclination, ngeo, distance, E, M, h, chunk, max_steps, backend, device, verbose)
