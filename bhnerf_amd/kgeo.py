"""bhnerf.kgeo hot-path member: the radiative-transfer ray integral (kgeo.py:595-622).

The reference spells it ``radiative_trasfer``; both spellings are exported.  Device tensors go
through the HIP kernel ``bhn_radiative_transfer_fwd``/``_bwd`` (differentiable w.r.t. emission);
NumPy inputs follow the reference's own NumPy path (``use_jax=False``).

The GR pre-compute part of bhnerf/kgeo.py is restated below on plain NumPy arrays (no xarray; 4-vectors
carry their component index ``mu = (t, r, theta, phi)`` on the LAST axis): ``image_plane_geos`` (own ray tracer,
``geodesics.py``), ``wave_vector``, ``spacetime_metric``, ``azimuthal_velocity_vector``, ``doppler_factor``,
``fluid_frame_tetrad``, ``magnetic_field_fluid_frame``, ``parallel_transport`` and the ZAMO variants
(kgeo.py:65-593).  ``geos`` is anything with attribute access to the fields of the reference's geodesic dataset
(``geodesics.Geodesics``, an ``xarray.Dataset`` of the real ``kgeo``, a ``types.SimpleNamespace`` ...).  Parity:
unpinned against the reference (its functions need xarray and the external ``kgeo``, neither is available); pinned
instead by the invariants they must satisfy -- ``u.u = -1``, ``k.k = 0``, orthonormal tetrads, the special-
relativistic Doppler factor far from the hole, conservation of the Penrose-Walker constant along a geodesic
(``tests/test_geodesics_cpu.py``).

``emission_factors`` is the chain ``alma.image_plane_model`` runs after the geodesics are traced (4-velocity -> Doppler factor ->
fluid-frame field -> its mean over the recovery domain -> parallel transport) as one function, on the host (``backend='numpy'``:
the functions above, composed) or on the GPU (``backend='hip'``: ``libbhnerf_grf.so``, include/bhnerf_grf.h).  With
``flow=`` it takes a general 4-velocity instead -- a ``umu`` array, or the boosted ZAMO of ``zamo_frame_velocity`` -- and
``frame='zamo'`` transports in the ZAMO tetrad (``parallel_transport_zamo``); on the GPU that is ``libbhnerf_flow.so``,
include/bhnerf_flow.h, DESIGN.md 4.13.
"""
import numpy as np
import torch

from . import _hip, utils


def _plane_shape(emission, *vs):
    """Shape (*spatial, G) of the per-ray factors: the first array-valued factor decides, else the
    trailing (H, W, G) axes of the emission."""
    for v in vs:
        if np.ndim(v) > 0:
            return tuple(v.shape)
    return tuple(emission.shape[-3:]) if emission.ndim >= 3 else tuple(emission.shape)


class _RadiativeTransfer(torch.autograd.Function):
    """img[n, r] = sum_k g^2 e[n, r, k] dtau Sigma through the C ABI (fwd and bwd kernels)."""

    @staticmethod
    def forward(ctx, emission, g, dtau, Sigma):
        full = tuple(g.shape)
        G, R = full[-1], int(np.prod(full[:-1]))
        lead = tuple(emission.shape[:emission.ndim - len(full)])
        N = int(np.prod(lead)) if lead else 1
        out = torch.empty(lead + full[:-1], dtype=torch.float32, device=emission.device)
        _hip.check(_hip.lib().bhn_radiative_transfer_fwd(
            _hip.ptr(emission), _hip.ptr(g), _hip.ptr(dtau), _hip.ptr(Sigma), _hip.ptr(out), N, R, G,
            _hip.stream_ptr(emission.device)))
        ctx.save_for_backward(g, dtau, Sigma)
        ctx.dims = (tuple(emission.shape), N, R, G)
        return out

    @staticmethod
    def backward(ctx, dimg):
        g, dtau, Sigma = ctx.saved_tensors
        eshape, N, R, G = ctx.dims
        de = torch.empty(eshape, dtype=torch.float32, device=dimg.device)
        _hip.check(_hip.lib().bhn_radiative_transfer_bwd(
            _hip.ptr(dimg.contiguous()), _hip.ptr(g), _hip.ptr(dtau), _hip.ptr(Sigma), _hip.ptr(de), N, R, G,
            _hip.stream_ptr(dimg.device)))
        return de, None, None, None


def radiative_trasfer(emission, g, dtau, Sigma, use_jax=False):
    """stokes = sum_k g^2 * emission * dtau * Sigma over the last (geodesic-sample) axis."""
    if isinstance(emission, torch.Tensor):
        _hip.require_device(emission)
        full = _plane_shape(emission, g, dtau, Sigma)
        dev = emission.device
        planes = [_hip.as_f32(v, dev).expand(full).contiguous() for v in (g, dtau, Sigma)]
        return _RadiativeTransfer.apply(emission.to(torch.float32).contiguous(), *planes)
    nd = np.ndim(emission)
    g, dtau, Sigma = (utils.expand_dims(v, nd) for v in (g, dtau, Sigma))
    return (g ** 2 * emission * dtau * Sigma).sum(axis=-1)


radiative_transfer = radiative_trasfer


# ---------------------------------------------------------------------------------------------------------------
# GR pre-compute on NumPy arrays
# ---------------------------------------------------------------------------------------------------------------
from .geodesics import Geodesics, image_plane_geos, kerr_functions, ray_geos  # noqa: E402,F401
from . import equatorial_lensing  # noqa: E402,F401  (kgeo.equatorial_lensing.r_equatorial / rho_of_req, as the reference spells them)


def _f(geos, name):
    return np.asarray(getattr(geos, name), dtype=np.float64)


def transform_coordinates(v, tetrad, contraction):
    """``tetrad @ v`` over the last axis (kgeo.py:65-90); ``contraction='upper'`` uses the transposed tetrad."""
    v = np.asarray(v)
    if contraction == 'upper':
        tetrad = np.swapaxes(tetrad, -1, -2)
    elif contraction != 'lower':
        raise AttributeError('contraction can be either "upper" or "lower"')
    return np.einsum('...ij,...j->...i', tetrad, v)


def wave_vector(geos):
    """Covariant photon momentum ``k_mu = (-E, +-E sqrt(R)/Delta, +-E sqrt(Theta), E lam)`` (kgeo.py:92-116); the
    signs follow the direction of motion along the affine parameter (turning points)."""
    r, th, aff = _f(geos, 'r'), _f(geos, 'theta'), _f(geos, 'affine')
    E = _f(geos, 'E')
    lam = _f(geos, 'lam')
    if lam.ndim == r.ndim - 1:
        lam = lam[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        pm_r = np.sign(np.gradient(r, axis=-1) / np.gradient(aff, axis=-1))
        pm_th = np.sign(np.gradient(th, axis=-1) / np.gradient(aff, axis=-1))
    k_t = -E * np.ones_like(r)
    k_r = E * np.sqrt(np.clip(_f(geos, 'R'), 0.0, None)) * pm_r / _f(geos, 'Delta')
    k_th = E * np.sqrt(np.clip(_f(geos, 'Theta'), 0.0, None)) * pm_th
    k_ph = E * lam * np.ones_like(r)
    return np.stack([k_t, k_r, k_th, k_ph], axis=-1)


def spacetime_metric(geos):
    """Non-zero covariant Kerr metric components in Boyer-Lindquist coordinates (kgeo.py:118-144)."""
    r, th, M, a = _f(geos, 'r'), _f(geos, 'theta'), _f(geos, 'M'), _f(geos, 'spin')
    Sg, Dl, Xi = _f(geos, 'Sigma'), _f(geos, 'Delta'), _f(geos, 'Xi')
    s2 = np.sin(th) ** 2
    return Geodesics(tt=-(1.0 - 2.0 * M * r / Sg), rr=Sg / Dl, thth=Sg, phph=Xi * s2 / Sg, tph=-2.0 * M * a * r * s2 / Sg)


def spacetime_inv_metric(geos):
    """Non-zero contravariant components (kgeo.py:146-173)."""
    r, th, M, a = _f(geos, 'r'), _f(geos, 'theta'), _f(geos, 'M'), _f(geos, 'spin')
    Sg, Dl, Xi = _f(geos, 'Sigma'), _f(geos, 'Delta'), _f(geos, 'Xi')
    s2 = np.sin(th) ** 2
    return Geodesics(tt=-Xi / (Dl * Sg), rr=Dl / Sg, thth=1.0 / Sg, phph=(Dl - a ** 2 * s2) / (Dl * Sg * s2),
                     tph=-2.0 * M * a * r / (Dl * Sg))


def raise_or_lower_indices(g, u):
    """``g_{mu nu} u^nu`` (or the inverse) for the block-diagonal + t-phi metric (kgeo.py:175-197)."""
    u = np.asarray(u)
    return np.stack([g.tt * u[..., 0] + g.tph * u[..., 3], g.rr * u[..., 1], g.thth * u[..., 2],
                     g.phph * u[..., 3] + g.tph * u[..., 0]], axis=-1)


def azimuthal_velocity_vector(geos, Omega):
    """Contravariant 4-velocity of matter on circular orbits with angular velocity ``Omega`` (kgeo.py:199-223)."""
    g = spacetime_metric(geos)
    Omega = np.asarray(Omega, dtype=np.float64) * np.ones_like(g.tt)
    with np.errstate(invalid='ignore', divide='ignore'):              # superluminal Omega -> NaN, as in the reference
        ut = 1.0 / np.sqrt(-(g.tt + 2.0 * Omega * g.tph + g.phph * Omega ** 2))
    zero = np.zeros_like(ut)
    return np.stack([ut, zero, zero, ut * Omega], axis=-1)


def doppler_factor(geos, umu, fillna=0.0):
    """``g = E / -(k_mu u^mu)`` (kgeo.py:225-248); NaNs (superluminal Omega) are replaced by ``fillna`` unless it is
    False or None."""
    g = _f(geos, 'E') / -(wave_vector(geos) * np.asarray(umu)).sum(axis=-1)
    if not ((isinstance(fillna, bool) and fillna is False) or fillna is None):
        g = np.where(np.isnan(g), fillna, g)
    return g


def magnetic_field_spherical(geos, b_r, b_th, b_ph):
    """A (r, theta, phi) field sampled on the geodesics; scalars are broadcast (kgeo.py:250-272)."""
    one = np.ones_like(_f(geos, 'r'))
    return np.stack([np.asarray(b_r) * one, np.asarray(b_th) * one, np.asarray(b_ph) * one], axis=-1)


def fluid_frame_tetrad(geos, umu):
    """Tetrad ``e[..., mu, a]`` (component index, then leg: the reference's layout) of the frame co-moving with
    ``umu`` (kgeo.py:310-345)."""
    g = spacetime_metric(geos)
    umu = np.asarray(umu)
    u_mu = raise_or_lower_indices(g, umu)
    uu = u_mu * umu
    th, Dl = _f(geos, 'theta'), _f(geos, 'Delta')
    tph = uu[..., 0] + uu[..., 3]
    N_r = np.sqrt(-g.rr * tph * (1.0 + uu[..., 2]))
    N_th = np.sqrt(g.thth * (1.0 + uu[..., 2]))
    N_ph = np.sqrt(-tph * Dl * np.sin(th) ** 2)
    zero = np.zeros_like(N_r)
    e_t = -umu
    e_r = np.stack([u_mu[..., 1] * umu[..., 0], -tph, zero, u_mu[..., 1] * umu[..., 3]], axis=-1) / N_r[..., None]
    e_th = np.stack([u_mu[..., 2] * umu[..., 0], u_mu[..., 2] * umu[..., 1], 1.0 + uu[..., 2], u_mu[..., 2] * umu[..., 3]],
                    axis=-1) / N_th[..., None]
    e_ph = np.stack([u_mu[..., 3], zero, zero, -u_mu[..., 0]], axis=-1) / N_ph[..., None]
    return np.stack([e_t, e_r, e_th, e_ph], axis=-1)


def magnetic_field_fluid_frame(geos, umu, arad, avert, ator):
    """Lab-frame field (radial / vertical / toroidal amplitudes) seen in the fluid frame (kgeo.py:274-308)."""
    th = _f(geos, 'theta')
    Br = arad * np.sin(th) + avert * np.cos(th)
    Bth = avert * (-np.sin(th))
    Bph = ator * np.ones_like(th)
    g = spacetime_metric(geos)
    umu = np.asarray(umu)
    u_mu = raise_or_lower_indices(g, umu)
    e = fluid_frame_tetrad(geos, umu)
    b0 = Br * u_mu[..., 1] + Bth * u_mu[..., 2] + Bph * u_mu[..., 3]
    b1 = (Br + b0 * u_mu[..., 1]) / u_mu[..., 0]
    b2 = (Bth + b0 * u_mu[..., 2]) / u_mu[..., 0]
    b3 = (Bph + b0 * u_mu[..., 3]) / u_mu[..., 0]
    b_mu = raise_or_lower_indices(g, np.stack([b0, b1, b2, b3], axis=-1))
    return transform_coordinates(b_mu, e, 'upper')[..., 1:]


def zamo_frame_velocity(geos, beta, chi):
    """Velocity of an observer boosted by ``beta`` at angle ``chi`` relative to the ZAMO (kgeo.py:408-436)."""
    r, Dl, Xi, om = _f(geos, 'r'), _f(geos, 'Delta'), _f(geos, 'Xi'), _f(geos, 'omega')
    gam = 1.0 / np.sqrt(1.0 - beta ** 2)
    ut = (gam / r) * np.sqrt(Xi / Dl)
    ur = (beta * gam * np.cos(chi) / r) * np.sqrt(Dl)
    uph = ut * om + r * beta * gam * np.sin(chi) / np.sqrt(Xi)
    return np.stack([ut, ur, np.zeros_like(ut), uph], axis=-1)


def zamo_frame_tetrad(geos, beta, chi):
    """Tetrad of the boosted ZAMO frame, Gelles et al. 2021 eq. A4 (kgeo.py:347-406)."""
    r, Dl, Xi, om = _f(geos, 'r'), _f(geos, 'Delta'), _f(geos, 'Xi'), _f(geos, 'omega')
    gam = 1.0 / np.sqrt(1.0 - beta ** 2)
    c, s = np.cos(chi), np.sin(chi)
    sxd, sd, sx = np.sqrt(Xi / Dl), np.sqrt(Dl), np.sqrt(Xi)
    zero = np.zeros_like(r)
    e_t = np.stack([(gam / r) * sxd, (beta * gam * c / r) * sd, zero, (gam * om / r) * sxd + r * beta * gam * s / sx], axis=-1)
    e_r = np.stack([(beta * gam * c / r) * sxd, ((1.0 + (gam - 1.0) * c ** 2) / r) * sd, zero,
                    beta * gam * om * c / r * sxd + r * (gam - 1.0) * c * s / sx], axis=-1)
    e_th = np.stack([zero, zero, 1.0 / r, zero], axis=-1)
    e_ph = np.stack([(beta * gam * s / r) * sxd, ((gam - 1.0) * c * s / r) * sd, zero,
                     beta * om * s * (gam / r) * sxd + r * ((gam - 1.0) * s ** 2 + 1.0) / sx], axis=-1)
    return np.stack([e_t, e_r, e_th, e_ph], axis=-1)


def _transport(geos, e_mu, g, b, Q_frac, V_frac, spectral_index, with_v):
    """Common part of parallel_transport / parallel_transport_zamo (kgeo.py:438-593): local EVPA from k x B in the
    emitter frame, emissivity scalings, rotation to the observer screen through the Penrose-Walker constant
    (Himwich et al. 2020)."""
    if Q_frac > 1.0 or Q_frac < 0.0:
        raise AttributeError('Q_frac should be in [0,1]')
    b = np.asarray(b, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    k_mu = wave_vector(geos)
    k_loc = transform_coordinates(k_mu, e_mu, 'upper')[..., 1:]
    k_mag = np.sqrt((k_loc ** 2).sum(axis=-1))
    f_loc = np.cross(k_loc, b, axis=-1) / k_mag[..., None]
    f_glob = transform_coordinates(np.concatenate([np.zeros_like(f_loc[..., :1]), f_loc], axis=-1), e_mu, 'lower')
    ft, fr, fth, fph = (f_glob[..., i] for i in range(4))
    b_mag = np.sqrt((b ** 2).sum(axis=-1))
    sin_b = np.sqrt((f_loc ** 2).sum(axis=-1)) / k_mag
    I = g ** spectral_index * b_mag ** (spectral_index + 1) * sin_b ** (spectral_index + 1)
    Q = Q_frac * I
    r, th, a = _f(geos, 'r'), _f(geos, 'theta'), _f(geos, 'spin')
    kup = raise_or_lower_indices(spacetime_inv_metric(geos), k_mu)
    s2 = np.sin(th) ** 2
    A = (kup[..., 0] * fr - kup[..., 1] * ft) + a * s2 * (kup[..., 1] * fph - kup[..., 3] * fr)
    B = ((r ** 2 + a ** 2) * (kup[..., 3] * fth - kup[..., 2] * fph) - a * (kup[..., 0] * fth - kup[..., 2] * ft)) * np.sin(th)
    kappa = (r - 1j * a * np.cos(th)) * (A - 1j * B)
    alpha, beta = _f(geos, 'alpha'), _f(geos, 'beta')
    if alpha.ndim == r.ndim - 1:
        alpha, beta = alpha[..., None], beta[..., None]
    mu = -(alpha + a * np.sin(_f(geos, 'inc')))
    with np.errstate(divide='ignore', invalid='ignore'):
        chi2 = np.angle(((beta + 1j * mu) * kappa.conj()) / ((beta - 1j * mu) * kappa))
    J = [I, np.cos(chi2) * Q, np.sin(chi2) * Q]                          # rot(chi2) applied to (Q, U = 0)
    if with_v:
        with np.errstate(divide='ignore', invalid='ignore'):
            cot_b = np.sqrt(1.0 - sin_b ** 2) / sin_b
            J.append(V_frac * g ** (-spectral_index - 0.5) * b_mag ** (spectral_index + 1.5) * sin_b ** (spectral_index + 1.5) * cot_b)
    return np.stack(J), kappa


def parallel_transport(geos, umu, g, b, Q_frac=0.2, V_frac=0.01, spectral_index=1):
    """Stokes scaling factors ``J = [I, Q, U(, V)]`` transported to the observer screen (kgeo.py:438-519); the V row
    is dropped when ``V_frac == 0``."""
    J, _ = _transport(geos, fluid_frame_tetrad(geos, umu), g, b, Q_frac, V_frac, spectral_index, V_frac != 0)
    return J


def parallel_transport_zamo(geos, beta_v, chi, g, b, Q_frac=0.2, spectral_index=1):
    """The same in the boosted ZAMO frame, ``J = [I, Q, U]`` (kgeo.py:521-593)."""
    J, _ = _transport(geos, zamo_frame_tetrad(geos, beta_v, chi), g, b, Q_frac, 0.0, spectral_index, False)
    return J


# ---------------------------------------------------------------------------------------------------------------
# Doppler factor and polarised transport factors of one hypothesis, on the host or on the GPU
# ---------------------------------------------------------------------------------------------------------------
_GRF_POINT_FIELDS = ('r', 'theta', 'affine', 'Delta', 'Sigma', 'Xi', 'R', 'Theta')
_GRF_RAY_FIELDS = ('lam', 'alpha', 'beta')


def _no_fill(fillna):
    return (isinstance(fillna, bool) and fillna is False) or fillna is None


def _emission_factors_numpy(geos, Omega, b_consts, domain, Q_frac, V_frac, spectral_index, fillna):
    umu = azimuthal_velocity_vector(geos, Omega)
    g = doppler_factor(geos, umu, fillna)
    if b_consts is None:
        return g, None
    b = magnetic_field_fluid_frame(geos, umu, **b_consts)
    if domain is not None:
        z_width, rmin, rmax = domain
        r = _f(geos, 'r')
        sel = (np.abs(r * np.cos(_f(geos, 'theta'))) < z_width) & (r > rmin) & (r < rmax)          # |z| of the record
        b = b / np.sqrt((b[sel] ** 2).sum(axis=-1)).mean()
    with np.errstate(divide='ignore', invalid='ignore'):
        J = parallel_transport(geos, umu, g, b, Q_frac=Q_frac, V_frac=V_frac, spectral_index=spectral_index)
    return g, J


def _is_resident(geos):
    from .geodesics import DeviceGeodesics
    return isinstance(geos, DeviceGeodesics)


def _shape(geos):
    """The shape of the record's per-point fields, without a copy of a resident record's."""
    return tuple(geos.r.shape) if _is_resident(geos) else _f(geos, 'r').shape


def _hip_device(geos, b_consts, Q_frac, lib, device):
    """What both device paths check before anything touches the device, in this order; the torch device (a resident record's own)."""
    shape = _shape(geos)
    if len(shape) < 1 or shape[-1] < 2:            # np.gradient's own error, before anything touches the device
        raise ValueError('Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.')
    if b_consts is not None and (Q_frac > 1.0 or Q_frac < 0.0):
        raise AttributeError('Q_frac should be in [0,1]')
    lib()
    if not torch.cuda.is_available():
        raise _hip.HipError("backend='hip' needs a HIP device (there is no CPU fallback; backend='numpy' computes the factors on the host)")
    if _is_resident(geos):
        if device is not None and torch.device(device) != geos.device and torch.device(device) != torch.device(geos.device.type):
            raise ValueError('the record lives on %s, not on %s' % (geos.device, device))
        return geos.device
    return torch.device('cuda' if device is None else device)


def _upload(v, shp, dev):
    if isinstance(v, torch.Tensor):              # already a tensor (a resident record's Omega, umu, field): no host copy
        return v.to(device=dev, dtype=torch.float64).expand(shp).contiguous()
    v = np.asarray(v, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(v if v.shape == shp else np.broadcast_to(v, shp).copy()), device=dev)


def _upload_record(geos, dev):
    """The fields of include/bhnerf_grf.h's record on the device and the struct that names them: (fields, bhn_grf_geos)."""
    shape = _f(geos, 'r').shape
    fields = {k: _upload(_f(geos, k), shape, dev) for k in _GRF_POINT_FIELDS}
    fields.update({k: _upload(_f(geos, k), shape[:-1], dev) for k in _GRF_RAY_FIELDS})
    rec = _hip.bhn_grf_geos(_f(geos, 'r').size // shape[-1], shape[-1], *[fields[k].data_ptr() for k in _GRF_POINT_FIELDS + _GRF_RAY_FIELDS],
                            float(_f(geos, 'spin')), float(_f(geos, 'M')), float(_f(geos, 'E')), float(_f(geos, 'inc')))
    return fields, rec


def _resident_fields(geos, dev):
    """_upload_record for a DeviceGeodesics: the struct names the record's own buffers, nothing is copied."""
    shape = _shape(geos)
    fields = {k: _upload(geos[k], shape, dev) for k in _GRF_POINT_FIELDS}
    fields.update({k: _upload(geos[k], shape[:-1], dev) for k in _GRF_RAY_FIELDS})
    rec = _hip.bhn_grf_geos(fields['r'].numel() // shape[-1], shape[-1], *[fields[k].data_ptr() for k in _GRF_POINT_FIELDS + _GRF_RAY_FIELDS],
                            float(geos.spin), float(geos.M), float(geos.E), float(geos.inc))
    return fields, rec


def _domain_mean_hip(rec, b, domain, dev, stream):
    """bhn_grf_domain_mean on the device buffers of `rec`: the mean of |b| over the domain, one float64 on the device."""
    import ctypes as C
    lib = _hip.grf_lib()
    z_width, rmin, rmax = (float(v) for v in domain)
    nbytes = int(lib.bhn_grf_ws_bytes(rec.n, rec.ngeo))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    mean = torch.empty((1,), dtype=torch.float64, device=dev)
    _hip.grf_check(lib.bhn_grf_domain_mean(C.byref(rec), _hip.ptr(b), z_width, rmin, rmax, _hip.ptr(mean), _hip.ptr(ws), nbytes, stream))
    return mean


def _emission_factors_hip(geos, Omega, b_consts, domain, Q_frac, V_frac, spectral_index, fillna, device):
    """The calls of include/bhnerf_grf.h on one record: fields uploaded once, g (and J) downloaded.  A resident record
    (geodesics.DeviceGeodesics) is read where it is and g (and J) stay on its device."""
    import ctypes as C
    dev = _hip_device(geos, b_consts, Q_frac, _hip.grf_lib, device)
    lib = _hip.grf_lib()
    shape = _shape(geos)
    resident = _is_resident(geos)
    with torch.cuda.device(dev):
        fields, rec = _resident_fields(geos, dev) if resident else _upload_record(geos, dev)      # `fields` owns the buffers `rec` points into
        Om = _upload(Omega, shape, dev)
        stream = _hip.stream_ptr(dev)
        g = torch.empty(shape, dtype=torch.float64, device=dev)
        no_fill = _no_fill(fillna)
        _hip.grf_check(lib.bhn_grf_doppler(C.byref(rec), _hip.ptr(Om), 0.0 if no_fill else float(fillna), 0 if no_fill else 1, _hip.ptr(g), stream))
        if b_consts is None:
            return (g, None) if resident else (g.cpu().numpy(), None)
        b = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        _hip.grf_check(lib.bhn_grf_fluid_field(C.byref(rec), _hip.ptr(Om), float(b_consts['arad']), float(b_consts['avert']),
                                               float(b_consts['ator']), _hip.ptr(b), stream))
        mean = None if domain is None else _domain_mean_hip(rec, b, domain, dev, stream)
        S = 4 if V_frac != 0 else 3
        J = torch.empty((S,) + shape, dtype=torch.float64, device=dev)
        _hip.grf_check(lib.bhn_grf_transport(C.byref(rec), _hip.ptr(Om), _hip.ptr(g), _hip.ptr(b), _hip.ptr(mean), float(Q_frac), float(V_frac),
                                             float(spectral_index), _hip.ptr(J), stream))
        return (g, J) if resident else (g.cpu().numpy(), J.cpu().numpy())


# ---- a general 4-velocity: a umu array per point, or the boosted ZAMO

def _parse_flow(geos, flow, frame):
    """``flow`` and ``frame`` of emission_factors -> (zamo, umu): ``zamo = (beta, chi)``, scalars as given, for the device functions,
    or ``umu``, an array of the record's shape + (4,) (a tensor given with a resident record stays a tensor)."""
    shape = _shape(geos)
    if frame not in ('fluid', 'zamo'):
        raise ValueError("frame must be 'fluid' or 'zamo', not %r" % (frame,))
    if isinstance(flow, tuple) and len(flow) == 3 and isinstance(flow[0], str):
        if flow[0] != 'zamo':
            raise ValueError("flow must be ('zamo', beta, chi) or a umu array, not a %r flow" % (flow[0],))
        beta, chi = flow[1], flow[2]
        if np.ndim(beta) == 0 and np.ndim(chi) == 0:
            return (beta, chi), None
        if np.broadcast(np.empty(shape), beta, chi).shape != shape:
            raise ValueError('per-point beta and chi must have the shape of the record, %s' % (shape,))
        if _is_resident(geos):
            raise ValueError('per-point beta and chi are evaluated by the NumPy functions: give them the record\'s .numpy()')
        zamo, umu = None, zamo_frame_velocity(geos, beta, chi)
    else:
        zamo, umu = None, (flow if isinstance(flow, torch.Tensor) else np.asarray(flow, dtype=np.float64))
        if tuple(umu.shape) != shape + (4,):
            raise ValueError('flow must be (\'zamo\', beta, chi) or a umu array of shape %s, not %s' % (shape + (4,), tuple(umu.shape)))
    if frame == 'zamo':
        raise ValueError("frame='zamo' needs a scalar ZAMO flow, flow=('zamo', beta, chi)")
    return zamo, umu


def _field_kind(b_consts):
    """'fluid' (arad, avert, ator: the field follows the flow), 'spherical' (b_r, b_th, b_ph) or 'array' ((..., 3), taken as it is)."""
    if isinstance(b_consts, dict):
        if set(b_consts) == {'arad', 'avert', 'ator'}:
            return 'fluid'
        if set(b_consts) == {'b_r', 'b_th', 'b_ph'}:
            return 'spherical'
        raise ValueError('b_consts must have the keys arad, avert, ator or b_r, b_th, b_ph, not %s' % sorted(b_consts))
    return 'array'


def _given_field(geos, b_consts, kind):
    shape = _shape(geos) + (3,)
    if isinstance(b_consts, torch.Tensor):
        return b_consts                          # (broadcast on the device by _upload)
    if kind == 'spherical' and _is_resident(geos):               # only the record's shape enters
        from types import SimpleNamespace
        return magnetic_field_spherical(SimpleNamespace(r=np.empty(shape[:-1])), **b_consts)
    b = magnetic_field_spherical(geos, **b_consts) if kind == 'spherical' else np.asarray(b_consts, dtype=np.float64)
    return b if b.shape == shape else np.broadcast_to(b, shape)


def _flow_factors_numpy(geos, zamo, umu, frame, b_consts, domain, Q_frac, V_frac, spectral_index, fillna):
    with np.errstate(divide='ignore', invalid='ignore'):
        if zamo is not None:
            umu = zamo_frame_velocity(geos, *zamo)
        g = doppler_factor(geos, umu, fillna)
        if b_consts is None:
            return g, None
        kind = _field_kind(b_consts)
        b = magnetic_field_fluid_frame(geos, umu, **b_consts) if kind == 'fluid' else _given_field(geos, b_consts, kind)
        if domain is not None:
            z_width, rmin, rmax = domain
            r = _f(geos, 'r')
            sel = (np.abs(r * np.cos(_f(geos, 'theta'))) < z_width) & (r > rmin) & (r < rmax)
            b = b / np.sqrt((b[sel] ** 2).sum(axis=-1)).mean()
        if frame == 'zamo':
            return g, parallel_transport_zamo(geos, zamo[0], zamo[1], g, b, Q_frac=Q_frac, spectral_index=spectral_index)
        return g, parallel_transport(geos, umu, g, b, Q_frac=Q_frac, V_frac=V_frac, spectral_index=spectral_index)


def _flow_factors_hip(geos, zamo, umu, frame, b_consts, domain, Q_frac, V_frac, spectral_index, fillna, device):
    """The calls of include/bhnerf_flow.h on one record: fields uploaded once, g (and J) downloaded.  The domain mean is
    bhn_grf_domain_mean on the same device buffers.  A resident record is read where it is and g (and J) stay on its device."""
    import ctypes as C
    kind = None if b_consts is None else _field_kind(b_consts)
    dev = _hip_device(geos, b_consts, Q_frac, _hip.flow_lib, device)
    lib = _hip.flow_lib()
    shape = _shape(geos)
    resident = _is_resident(geos)
    with torch.cuda.device(dev):
        fields, grf_rec = _resident_fields(geos, dev) if resident else _upload_record(geos, dev)
        fields['omega'] = _upload(geos.omega if resident else _f(geos, 'omega'), shape, dev)
        rec = _hip.bhn_flow_geos(*[getattr(grf_rec, k) for k, _ in _hip.bhn_grf_geos._fields_], fields['omega'].data_ptr())
        stream = _hip.stream_ptr(dev)
        if zamo is not None:
            beta, chi = float(zamo[0]), float(zamo[1])
            u = torch.empty(shape + (4,), dtype=torch.float64, device=dev)
            _hip.flow_check(lib.bhn_flow_zamo_velocity(C.byref(rec), beta, chi, _hip.ptr(u), stream))
        else:
            u = _upload(umu, shape + (4,), dev)
        g = torch.empty(shape, dtype=torch.float64, device=dev)
        no_fill = _no_fill(fillna)
        _hip.flow_check(lib.bhn_flow_doppler(C.byref(rec), _hip.ptr(u), 0.0 if no_fill else float(fillna), 0 if no_fill else 1, _hip.ptr(g), stream))
        if b_consts is None:
            return (g, None) if resident else (g.cpu().numpy(), None)
        if kind == 'fluid':
            b = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
            _hip.flow_check(lib.bhn_flow_fluid_field(C.byref(rec), _hip.ptr(u), float(b_consts['arad']), float(b_consts['avert']),
                                                     float(b_consts['ator']), _hip.ptr(b), stream))
        else:
            b = _upload(_given_field(geos, b_consts, kind), shape + (3,), dev)
        mean = None if domain is None else _domain_mean_hip(grf_rec, b, domain, dev, stream)
        if frame == 'zamo':
            J = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
            _hip.flow_check(lib.bhn_flow_transport_zamo(C.byref(rec), beta, chi, _hip.ptr(g), _hip.ptr(b), _hip.ptr(mean), float(Q_frac),
                                                        float(spectral_index), _hip.ptr(J), stream))
        else:
            J = torch.empty(((4 if V_frac != 0 else 3),) + shape, dtype=torch.float64, device=dev)
            _hip.flow_check(lib.bhn_flow_transport(C.byref(rec), _hip.ptr(u), _hip.ptr(g), _hip.ptr(b), _hip.ptr(mean), float(Q_frac),
                                                   float(V_frac), float(spectral_index), _hip.ptr(J), stream))
        return (g, J) if resident else (g.cpu().numpy(), J.cpu().numpy())


def emission_factors(geos, Omega=None, b_consts=None, domain=None, Q_frac=0.2, V_frac=0.01, spectral_index=1, fillna=0.0, backend='numpy',
                     device=None, flow=None, frame='fluid'):
    """Doppler factor ``g`` and polarised transport factors ``J`` of one hypothesis about the emitting matter.  Returns ``(g, J)``;
    ``J`` is None when ``b_consts`` is None.  ``domain=(z_width, rmin, rmax)`` divides the field by its mean magnitude over the
    points with ``|z| < z_width, rmin < r < rmax``; None leaves it as it is.

    The 4-velocity is given by exactly one of ``Omega`` and ``flow`` (both, or neither, is a ``ValueError``):

    * ``Omega``: matter on circular orbits with that angular velocity, ``azimuthal_velocity_vector -> doppler_factor ->
      magnetic_field_fluid_frame -> (domain mean) -> parallel_transport``, what ``alma.image_plane_model`` computes after the
      geodesics are traced; ``b_consts`` is ``dict(arad, avert, ator)``.
    * ``flow=('zamo', beta, chi)``: the boosted ZAMO of ``zamo_frame_velocity`` (Gelles et al. 2021).  Scalars go to the device
      function; per-point arrays of the record's shape are evaluated on the host and taken as a ``umu`` array.
    * ``flow=`` an array of shape ``geos.r.shape + (4,)``: a general ``umu`` per point.

    With a ``flow``, ``b_consts`` is ``dict(arad, avert, ator)`` (``magnetic_field_fluid_frame`` of the flow),
    ``dict(b_r, b_th, b_ph)`` (``magnetic_field_spherical``) or an array ``(..., 3)`` taken as it is, and ``frame`` chooses the
    tetrad of the transport: ``'fluid'`` is ``parallel_transport(geos, umu, ...)``; ``'zamo'`` is ``parallel_transport_zamo``,
    which needs a scalar ZAMO flow (anything else is a ``ValueError``), ignores ``V_frac`` and returns three rows.

    ``backend='numpy'`` (the default) composes the functions above on the host.  ``'hip'`` uploads the fields of the record once and
    makes the calls of ``include/bhnerf_grf.h`` (``Omega``; ``libbhnerf_grf.so``, csrc/gr_factors.hip) or ``include/bhnerf_flow.h``
    (``flow``; ``libbhnerf_flow.so``, csrc/flow_factors.hip) -- the same expressions, one GPU lane per sample point -- on ``device``
    (a torch device, default the current one); float64 NumPy arrays of the same shapes come back.  There is no CPU fallback:
    ``'hip'`` without a device raises ``HipError``.

    A resident record (``geodesics.DeviceGeodesics``, ``image_plane_geos(..., backend='hip', resident=True)``) needs
    ``backend='hip'``: the libraries read the record's own device buffers, ``Omega``, a ``umu`` array and a given field may be tensors
    or arrays, and ``(g, J)`` come back as float64 tensors on the record's device."""
    from .geodesics import _check_backend
    _check_backend(backend)
    if _is_resident(geos) and backend != 'hip':
        raise ValueError("a resident record (DeviceGeodesics) needs backend='hip'; the NumPy functions take its .numpy()")
    if (Omega is None) == (flow is None):
        raise ValueError('give exactly one of Omega and flow (%s were given)' % ('both' if flow is not None else 'neither'))
    if flow is None:
        if frame != 'fluid':
            raise ValueError("frame=%r needs a scalar ZAMO flow, flow=('zamo', beta, chi)" % (frame,))
        if backend == 'hip':
            return _emission_factors_hip(geos, Omega, b_consts, domain, Q_frac, V_frac, spectral_index, fillna, device)
        return _emission_factors_numpy(geos, Omega, b_consts, domain, Q_frac, V_frac, spectral_index, fillna)
    zamo, umu = _parse_flow(geos, flow, frame)
    if backend == 'hip':
        return _flow_factors_hip(geos, zamo, umu, frame, b_consts, domain, Q_frac, V_frac, spectral_index, fillna, device)
    return _flow_factors_numpy(geos, zamo, umu, frame, b_consts, domain, Q_frac, V_frac, spectral_index, fillna)
