"""Inputs, the NumPy reference and the conditions of the general-flow (g, J) tests (libbhnerf_flow.so, kgeo.emission_factors with
flow=), shared by tests/test_flow_factors_cpu.py and tests/test_gpu_flow_factors.py.

The reference is the NumPy code of bhnerf_amd/kgeo.py composed here as the polarised-ring study composes it: zamo_frame_velocity (or a
umu array) -> doppler_factor -> magnetic_field_spherical / magnetic_field_fluid_frame -> parallel_transport (the fluid tetrad of umu)
and parallel_transport_zamo (the boosted ZAMO tetrad).  It does not go through kgeo.emission_factors.

Records, domain, metric and bound are those of tests/gr_factor_cases.py (10 x 7 rays x 40 samples, 2,800 points: 10 full workgroups
and a tail of 240; 'tiny' is one ray of 3 samples; NaN and inf patterns identical at every point; GR_TOL = 1e-10 relative to
max(|want|, largest in-domain |want|) per plane).  The domain only selects the points of that metric and of the conditions; the field is
divided by a scalar only where a test says so.

Cases: Z1-Z4 and Zt are scalar (beta, chi) settings, which reach the device functions; Za (a smooth per-point beta and chi), Zs (beta =
1.2 inside r < 3: superluminal, NaN points) and Zk (the Keplerian azimuthal 4-velocity of gr_factor_cases' case A) are handed over as umu
arrays.

Conditions (assert_conditions), from the NumPy values alone: Delta > 0 at every point; except in Zs no NaN or inf in g anywhere (Zk, whose
Keplerian flow is superluminal next to the horizon, is held to the conditions of gr_factor_cases' case A instead), no NaN in b or in the I, Q, U rows (both frames) inside the domain, at least 300 points there (2 in Zt); where the V row is computed no point
nearer than 1e-5 to the edge sin_b = 1 of that row's NaN region and at least 300 finite V values in the domain; Zs has at least 100 NaN
points."""
import numpy as np

import gr_factor_cases as gc
from bhnerf_amd import kgeo

GR_TOL = gc.GR_TOL
Q_FRAC = gc.Q_FRAC

# name -> (record of gr_factor_cases.CASES, beta, chi, field kind, field); beta / chi None: a umu array, see flow_of
CASES = {
    'Z1': ('A', 0.5, -np.pi / 2, 'spherical', (0.87, 0.0, 0.5)),
    'Z2': ('C', 0.0, 0.0, 'spherical', (1.0, 0.0, 0.0)),                 # the pure ZAMO
    'Z3': ('D', 0.9, 0.7, 'fluid', (0.3, 0.5, 0.8)),
    'Z4': ('B', 0.3, 2.5, 'fluid', (0.0, 1.0, 0.0)),
    'Zt': ('tiny', 0.5, -np.pi / 2, 'spherical', (0.5, 0.0, 0.87)),
    'Za': ('A', None, None, 'spherical', (0.87, 0.0, 0.5)),
    'Zs': ('A', None, None, 'spherical', (0.87, 0.0, 0.5)),
    'Zk': ('A', None, None, 'fluid', (0.0, 1.0, 0.0)),
}
SCALAR = ('Z1', 'Z2', 'Z3', 'Z4', 'Zt')
# (case, V_frac, spectral_index): V_frac = 0 everywhere, and on Z1 the V row with a non-integer power
VARIANTS = [(name, 0.0, 1) for name in CASES] + [('Z1', 0.01, 1.5)]
MIN_IN_DOMAIN = {name: (2 if name == 'Zt' else 300) for name in CASES}
ZS_RADIUS = 3.0


def trace(name, backend='numpy', device=None):
    return gc.trace(CASES[name][0], backend=backend, device=device)


def domain_of(name):
    return gc.domain_of(CASES[name][0])


def per_point(name, geos):
    """(beta, chi) arrays of Za and Zs."""
    r, theta = np.asarray(geos.r), np.asarray(geos.theta)
    if name == 'Za':
        return np.clip(0.2 + 0.05 * r / 9.0, 0.0, 0.9), -np.pi / 2 + 0.1 * np.cos(theta)
    assert name == 'Zs'
    return np.where(r < ZS_RADIUS, 1.2, 0.4), np.full(r.shape, -np.pi / 2)


def b_consts_of(name):
    _, _, _, kind, field = CASES[name]
    return dict(zip(('b_r', 'b_th', 'b_ph') if kind == 'spherical' else ('arad', 'avert', 'ator'), field))


def reference(name, geos, V_frac=0.0, spectral_index=1, divisor=None):
    """The composed NumPy functions on one record: a dict with flow (what emission_factors takes), umu, g (fillna 0), g_nan (fillna
    False), b (not divided), J (fluid tetrad, of b / divisor), J_zamo (scalar cases), the domain mask and the distance of every point
    from the edge of the V row's NaN region."""
    record, beta, chi, kind, field = CASES[name]
    z_width, rmin, rmax = domain_of(name)
    with np.errstate(divide='ignore', invalid='ignore'):
        if name in SCALAR:
            umu, flow = kgeo.zamo_frame_velocity(geos, beta, chi), ('zamo', beta, chi)
        elif name == 'Zk':
            umu = kgeo.azimuthal_velocity_vector(geos, gc.keplerian(geos, gc.CASES[record][2]))
            flow = umu
        else:
            umu = kgeo.zamo_frame_velocity(geos, *per_point(name, geos))
            flow = umu
        g = kgeo.doppler_factor(geos, umu)
        g_nan = kgeo.doppler_factor(geos, umu, fillna=False)
        b = kgeo.magnetic_field_spherical(geos, *field) if kind == 'spherical' else kgeo.magnetic_field_fluid_frame(geos, umu, *field)
        bd = b if divisor is None else b / divisor
        J = kgeo.parallel_transport(geos, umu, g, bd, Q_frac=Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)
        J_zamo = None
        if name in SCALAR:
            J_zamo = kgeo.parallel_transport_zamo(geos, beta, chi, g, bd, Q_frac=Q_FRAC, spectral_index=spectral_index)
        k_loc = kgeo.transform_coordinates(kgeo.wave_vector(geos), kgeo.fluid_frame_tetrad(geos, umu), 'upper')[..., 1:]
        k2 = (k_loc ** 2).sum(axis=-1)
        sin_b = np.sqrt((np.cross(k_loc, bd, axis=-1) ** 2).sum(axis=-1)) / k2
        v_margin = np.abs(1.0 - sin_b ** 2)
    domain = (np.abs(geos.z) < z_width) & (geos.r > rmin) & (geos.r < rmax)
    return dict(flow=flow, umu=umu, g=g, g_nan=g_nan, b=b, J=J, J_zamo=J_zamo, domain=domain, v_margin=v_margin, divisor=divisor)


def domain_mean(ref):
    """The mean of |b| over the domain, from the reference's field."""
    return float(np.sqrt((ref['b'][ref['domain']] ** 2).sum(axis=-1)).mean())


def assert_conditions(name, geos, ref):
    """What the comparison relies on, from the NumPy values alone."""
    dom = ref['domain']
    assert dom.sum() >= MIN_IN_DOMAIN[name], (name, int(dom.sum()))
    assert np.asarray(geos.Delta).min() > 0.0, (name, np.asarray(geos.Delta).min())
    if name == 'Zs':
        assert np.isnan(ref['g_nan']).sum() >= 100, int(np.isnan(ref['g_nan']).sum())
        assert not np.isnan(ref['g']).any()
        return
    if name != 'Zk':                                                  # (the Keplerian flow is superluminal next to the horizon)
        assert np.isfinite(ref['g_nan']).all(), name
    assert not np.isnan(ref['b'][dom]).any() and not np.isnan(ref['J'][:3, dom]).any(), name
    if ref['J_zamo'] is not None:
        assert ref['J_zamo'].shape[0] == 3 and not np.isnan(ref['J_zamo'][:, dom]).any(), name
    if ref['J'].shape[0] == 4:
        assert np.nanmin(ref['v_margin']) >= 1e-5, (name, np.nanmin(ref['v_margin']))
        assert np.isfinite(ref['J'][3][dom]).sum() >= 300, (name, int(np.isfinite(ref['J'][3][dom]).sum()))


def errors(ref, umu=None, g=None, g_nan=None, b=None, J=None, J_zamo=None):
    """The per-quantity figures of what is given, in the metric of gr_factor_cases: a dict name -> figure, each to be <= GR_TOL."""
    out = {}
    dom = ref['domain']
    if umu is not None:
        for i in range(4):
            out['u%d' % i] = gc.plane_error(umu[..., i], ref['umu'][..., i], dom, 'umu[%d]' % i)
    for key, got in (('g', g), ('g_nan', g_nan)):
        if got is None:
            continue
        want = ref[key]
        gc.same_pattern(got, want, key)
        fin = np.isfinite(want)
        out[key] = float(np.abs(got[fin] - want[fin]).max() / np.abs(want[fin]).max())
    if b is not None:
        for i in range(3):
            out['b%d' % i] = gc.plane_error(b[..., i], ref['b'][..., i], dom, 'b[%d]' % i)
    for key, got in (('J', J), ('J_zamo', J_zamo)):
        if got is None:
            continue
        assert got.shape == ref[key].shape, (key, got.shape, ref[key].shape)
        for s in range(got.shape[0]):
            out['%s%d' % ('J' if key == 'J' else 'Jz', s)] = gc.plane_error(got[s], ref[key][s], dom, '%s[%d]' % (key, s))
    return out


def report(tag, name, V_frac, spectral_index, errs):
    print('\n[flow factors, %s] case %-3s V_frac %-4g index %-3g ' % (tag, name, V_frac, spectral_index)
          + '  '.join('%s %.1e' % (k, e) for k, e in errs.items()))
