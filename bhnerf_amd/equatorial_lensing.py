"""Equatorial lensing (``kgeo.equatorial_lensing`` of the external package the reference imports): which radius of the equatorial
plane a screen position shows in its direct image (``mbar = 0``), its first photon ring (``mbar = 1``), ..., and the inverse.

The reference reads two functions of that module: ``r_equatorial(...)[0:2]`` (emission.py:136) and ``rho_of_req(...)[-2:]`` (the
Gelles-2021 and ALMA-hotspot notebooks).  The external package evaluates closed forms in elliptic integrals; it is absent, so both
are built here on the project's own primitive, ``geodesics.equatorial_crossings``: the ``(mbar+1)``-th meeting of a ray of the
numeric tracer with the plane, on the host (``backend='numpy'``) or on the GPU (``backend='hip'``, ``bhn_eql_crossings``).
**Parity with the external ``kgeo`` is unpinned and stays so**: only the elements the reference reads are provided, and what is
checked instead are the closed forms of Gralla & Lupsasca the tracer is held to (tests/test_equatorial_cpu.py)."""
import numpy as np

from . import geodesics

DISTANCE_AT_INFINITY = 1000.0        # r_o = inf: the tracer's default observer distance
MAX_BISECTIONS = 200
DEFAULT_VARPHIS = np.linspace(-180.0, 179.0, 360) * np.pi / 180.0


def _distance(r_o):
    return DISTANCE_AT_INFINITY if np.isinf(r_o) else float(r_o)


def r_equatorial(a, r_o, th_o, mbar, alpha, beta, h=0.02, max_steps=400000, backend='numpy', device=None):
    """Radius and Mino time at which the rays ``(alpha, beta)`` of an observer at ``(r_o, th_o)`` of a hole of spin ``a`` (M = 1)
    meet the equatorial plane for the ``(mbar+1)``-th time: a tuple ``(r, mino)`` of arrays, one element per ray (NaN where a ray
    has no such crossing).  ``mino`` carries the sign convention of ``image_plane_geos`` (negative along the ray), so that
    ``abs(geos.mino - mino[:, None])`` is the distance of a record's samples from the crossing.  ``r_o = inf`` is the tracer's
    ``distance = 1000``.  Parity with the external ``kgeo.equatorial_lensing.r_equatorial`` is unpinned; elements ``[0]`` and ``[1]``
    are the only ones the reference reads."""
    mbar = int(mbar)
    if mbar < 0:
        raise ValueError('mbar must not be negative')
    alpha = np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel()
    beta = np.atleast_1d(np.asarray(beta, dtype=np.float64)).ravel()
    beta = np.where(beta == 0.0, 1e-9, beta)                  # (the nudge of image_plane_geos)
    c = geodesics.equatorial_crossings(alpha, beta, a, th_o, nmax=mbar + 1, distance=_distance(r_o), h=h, max_steps=max_steps,
                                       backend=backend, device=device)
    return c.r[:, mbar], c.mino[:, mbar]


def rho_of_req(a, th_o, req, mbar=0, varphis=None, distance=DISTANCE_AT_INFINITY, h=0.02, max_steps=400000, backend='numpy',
               device=None):
    """The screen positions that show the equatorial radius ``req`` in the image of order ``mbar``: for every image-plane angle of
    ``varphis`` the polar radius ``rho`` whose ray ``(rho cos varphi, rho sin varphi)`` meets the plane for the ``(mbar+1)``-th
    time at ``r = req``.  Returns ``(rho, varphis, alpha, beta)``; the reference reads ``[-2:]``.

    Bisection in ``rho`` along every angle, all angles in one batched crossings call per iteration (plus one batched end-state call
    for the rays that lack the crossing).  A ray is LOW when it is captured with fewer than ``mbar+1`` crossings or crosses at
    ``r < req``, HIGH when it escapes with fewer than ``mbar+1`` crossings or crosses at ``r > req``: every lensing band maps onto the
    whole plane, from the horizon at its inner edge to infinity at its outer one, so this classification is monotone in ``rho``.
    It runs until every bracket is narrower than ``1e-12 rho`` or MAX_BISECTIONS iterations are done.  Parity with the external
    ``kgeo.equatorial_lensing.rho_of_req`` is unpinned and stays so."""
    mbar = int(mbar)
    if mbar < 0:
        raise ValueError('mbar must not be negative')
    varphis = DEFAULT_VARPHIS if varphis is None else np.atleast_1d(np.asarray(varphis, dtype=np.float64)).ravel()
    req = np.broadcast_to(np.asarray(req, dtype=np.float64), varphis.shape)
    distance = float(distance)
    r_hor = 1.0 + np.sqrt(max(1.0 - float(a) ** 2, 0.0))
    if not ((req > 1.02 * r_hor).all() and (req < distance).all()):
        raise ValueError('req must lie between the horizon (1.02 r_hor) and the observer (distance)')
    cos_v, sin_v = np.cos(varphis), np.sin(varphis)

    def is_low(rho):
        alpha, beta = rho * cos_v, rho * sin_v
        beta = np.where(beta == 0.0, 1e-9, beta)
        c = geodesics.equatorial_crossings(alpha, beta, a, th_o, nmax=mbar + 1, distance=distance, h=h, max_steps=max_steps,
                                           backend=backend, device=device)
        low = c.r[:, mbar] < req                              # (False where the ray lacks the crossing: NaN)
        lacks = c.count <= mbar
        if lacks.any():
            _, end, _, _ = geodesics.trace(alpha[lacks], beta[lacks], a, th_o, distance=distance, h=h, max_steps=max_steps,
                                           backend=backend, device=device)
            low[lacks] = ~(end[0] > distance)                 # captured
        return low

    lo = np.full(varphis.shape, 1e-3)
    hi = 2.0 * req + 20.0
    if not (is_low(lo).all() and not is_low(hi).any()):
        raise RuntimeError('rho_of_req: the initial bracket does not hold req = %s at mbar = %d' % (np.unique(req), mbar))
    for _ in range(MAX_BISECTIONS):
        if ((hi - lo) <= 1e-12 * hi).all():
            break
        mid = 0.5 * (lo + hi)
        low = is_low(mid)
        lo, hi = np.where(low, mid, lo), np.where(low, hi, mid)
    rho = 0.5 * (lo + hi)
    return rho, varphis, rho * cos_v, rho * sin_v
