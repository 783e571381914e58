"""Inputs, the NumPy reference and the metric of the (g, J) tests (libbhnerf_grf.so, kgeo.emission_factors), shared by
tests/test_gr_factors_cpu.py and tests/test_gpu_gr_factors.py.

The reference is the NumPy code of bhnerf_amd/kgeo.py composed here as alma.image_plane_model composes it:
azimuthal_velocity_vector -> doppler_factor -> magnetic_field_fluid_frame -> mean of |b| over the recovery domain ->
parallel_transport.  It does not go through kgeo.emission_factors.

Records: 10 x 7 rays over (-9, 9)^2, 40 samples (2,800 points: 10 full workgroups of 256 and a tail of 240), domain z_width = 4,
rmin = isco_pro(spin), rmax = 9; Keplerian Omega = +-sqrt(M) / (r^1.5 + a sqrt(M)).  'tiny' is one ray of 3 samples (one-sided
differences only, fewer points than a wave), two of them inside the domain.

Conditions (assert_conditions), from the NumPy values alone: cases A-D have no NaN in b and in the I, Q, U rows inside the domain and
at least 300 points there; no point of theirs is nearer than 1e-5 to the timelike boundary g_tt + 2 Omega g_tphi + g_phiphi Omega^2 = 0
or, where the V row is computed, to the edge sin_b = 1 of the region where that row is NaN (rounding is 1e-16: it cannot decide NaN
versus not); case C has at least 100 superluminal NaN points; in case E the mean and every J are NaN.

Metric.  isnan and isinf patterns identical at every point.  g: |got - want| <= GR_TOL max|want|.  b (per component) and each plane of
J, per point: |got - want| <= GR_TOL max(|want|, m) with m the plane's largest in-domain |want| -- far from the hole J grows smoothly to
1e9..1e17 times its in-domain size, a bound relative to the global maximum would check nothing where the renderer reads.  The figures
returned are the largest |got - want| / that bound's right-hand side without GR_TOL, to be compared with GR_TOL = 1e-10 (the project's
bound, tests/test_geodesics_cpu.py); four-ulp noise on the input fields moves these cases by <= 2.6e-12 in this metric."""
import numpy as np

from bhnerf_amd import constants, kgeo

GR_TOL = 1e-10
FOV = ((-9.0, 9.0), (-9.0, 9.0))
NA, NB, NGEO = 10, 7, 40
Z_WIDTH, RMAX = 4.0, 9.0
Q_FRAC = 0.85
POINT_FIELDS = ('r', 'theta', 'affine', 'Delta', 'Sigma', 'Xi', 'R', 'Theta')
RAY_FIELDS = ('lam', 'alpha', 'beta')

# name -> (spin, inclination [deg], Omega direction, (arad, avert, ator))
CASES = {
    'A': (0.94, 60.0, 'ccw', (0.0, 1.0, 0.0)),
    'B': (0.94, 17.0, 'ccw', (0.3, 0.5, 0.8)),
    'C': (0.0, 60.0, 'cw', (0.0, 1.0, 0.0)),               # superluminal NaN points inside r < 3
    'D': (0.8, 90.0, 'ccw', (1.0, 0.0, 0.0)),
    'E': (0.94, 60.0, 'cw', (0.0, 1.0, 0.0)),              # a NaN inside the domain: the mean, hence every J, is NaN
    'tiny': (0.94, 60.0, 'ccw', (0.0, 1.0, 0.0)),
}
REGULAR = ('A', 'B', 'C', 'D')                              # no NaN inside the domain
# (V_frac, spectral_index) variants: the default of alma.image_plane_model, and on case B the V row with a non-integer power
VARIANTS = [(name, 0.0, 1) for name in CASES] + [('B', 0.01, 1.5)]
MIN_IN_DOMAIN = {'A': 300, 'B': 300, 'C': 300, 'D': 300, 'E': 300, 'tiny': 1}


def trace(name, backend='numpy', device=None):
    """The geodesic record of a case (NaNs filled with 0 as alma.image_plane_model does)."""
    spin, inc_deg = CASES[name][:2]
    if name == 'tiny':
        return kgeo.image_plane_geos(spin, np.deg2rad(inc_deg), (-6.0, -6.0), (2.0, 2.0), ngeo=3, num_alpha=1, num_beta=1, backend=backend,
                                     device=device).fillna(0.0)
    return kgeo.image_plane_geos(spin, np.deg2rad(inc_deg), FOV[0], FOV[1], ngeo=NGEO, num_alpha=NA, num_beta=NB, backend=backend,
                                 device=device).fillna(0.0)


def keplerian(geos, direction):
    sqrt_M = np.sqrt(geos.M)
    return {'cw': -1.0, 'ccw': 1.0}[direction] * sqrt_M / (geos.r ** 1.5 + geos.spin * sqrt_M)


def domain_of(name):
    return (Z_WIDTH, float(constants.isco_pro(CASES[name][0])), RMAX)


def reference(name, geos, V_frac=0.0, spectral_index=1):
    """The composed NumPy functions on one record: a dict with Omega, g (fillna 0), g_nan (fillna False), b (not normalised), mean,
    J (of b / mean), the domain mask and the distance of every point from the timelike boundary."""
    _, _, direction, (arad, avert, ator) = CASES[name]
    z_width, rmin, rmax = domain_of(name)
    Omega = keplerian(geos, direction)
    umu = kgeo.azimuthal_velocity_vector(geos, Omega)
    g = kgeo.doppler_factor(geos, umu)
    g_nan = kgeo.doppler_factor(geos, umu, fillna=False)
    with np.errstate(divide='ignore', invalid='ignore'):
        b = kgeo.magnetic_field_fluid_frame(geos, umu, arad, avert, ator)
        domain = (np.abs(geos.z) < z_width) & (geos.r > rmin) & (geos.r < rmax)
        mean = np.sqrt((b[domain] ** 2).sum(axis=-1)).mean()
        J = kgeo.parallel_transport(geos, umu, g, b / mean, Q_frac=Q_FRAC, V_frac=V_frac, spectral_index=spectral_index)
        # the V row holds sqrt(1 - sin_b^2) with parallel_transport's sin_b = |k x b| / |k|^2, which is not bounded by 1: the row is NaN
        # over a whole region, and v_margin is the distance of every point from that region's edge
        k_loc = kgeo.transform_coordinates(kgeo.wave_vector(geos), kgeo.fluid_frame_tetrad(geos, umu), 'upper')[..., 1:]
        k2 = (k_loc ** 2).sum(axis=-1)
        sin_b = np.sqrt((np.cross(k_loc, b / mean, axis=-1) ** 2).sum(axis=-1)) / k2
        v_margin = np.abs(1.0 - sin_b ** 2)
    m = kgeo.spacetime_metric(geos)
    margin = np.abs(m.tt + 2.0 * Omega * m.tph + m.phph * Omega ** 2)
    return dict(Omega=Omega, g=g, g_nan=g_nan, b=b, mean=mean, J=J, domain=domain, margin=margin, v_margin=v_margin)


def assert_conditions(name, ref):
    """What the comparison relies on, from the NumPy values alone."""
    dom = ref['domain']
    assert dom.sum() >= MIN_IN_DOMAIN[name], (name, int(dom.sum()))
    if name in REGULAR or name == 'tiny':
        assert not np.isnan(ref['b'][dom]).any() and not np.isnan(ref['J'][:3, dom]).any() and np.isfinite(ref['mean']), name
        assert ref['margin'].min() >= 1e-5, (name, ref['margin'].min())          # no point on the timelike boundary
        if ref['J'].shape[0] == 4:                                                # nor on the edge of the V row's NaN region
            assert np.nanmin(ref['v_margin']) >= 1e-5, (name, np.nanmin(ref['v_margin']))
            assert np.isfinite(ref['J'][3][dom]).sum() >= 300, (name, int(np.isfinite(ref['J'][3][dom]).sum()))
    if name == 'C':
        assert np.isnan(ref['g_nan']).sum() >= 100, int(np.isnan(ref['g_nan']).sum())
        assert not np.isnan(ref['g']).any()
    if name == 'E':
        assert np.isnan(ref['mean']) and np.isnan(ref['J']).all()


def same_pattern(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: %d NaN, %d wanted' % (what, np.isnan(got).sum(), np.isnan(want).sum())
    assert np.array_equal(np.isinf(got), np.isinf(want)), '%s: %d inf, %d wanted' % (what, np.isinf(got).sum(), np.isinf(want).sum())
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), '%s: sign of an inf' % what


def plane_error(got, want, domain, what):
    """max over the points of |got - want| / max(|want|, m), m the largest finite in-domain |want|; 0 for a plane without a finite point."""
    same_pattern(got, want, what)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    inside = np.abs(want[domain & fin])
    m = inside.max() if inside.size else 0.0
    scale = np.maximum(np.abs(want[fin]), m)
    err = np.abs(got[fin] - want[fin])
    return float(np.max(np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), np.where(err > 0.0, np.inf, 0.0))))


def errors(got_g, got_b, got_mean, got_J, ref, got_g_nan=None):
    """The per-quantity figures of one case in the metric of this module: a dict name -> figure, each to be <= GR_TOL."""
    out = {}
    for key, got in (('g', got_g), ('g_nan', got_g_nan)):
        if got is None:
            continue
        want = ref[key]
        same_pattern(got, want, key)
        fin = np.isfinite(want)
        out[key] = float(np.abs(got[fin] - want[fin]).max() / np.abs(want[fin]).max())
    for i in range(3):
        out['b%d' % i] = plane_error(got_b[..., i], ref['b'][..., i], ref['domain'], 'b[%d]' % i)
    same_pattern(np.float64(got_mean), np.float64(ref['mean']), 'mean')
    out['mean'] = float(abs(got_mean - ref['mean']) / abs(ref['mean'])) if np.isfinite(ref['mean']) else 0.0
    assert got_J.shape == ref['J'].shape, (got_J.shape, ref['J'].shape)
    for s in range(ref['J'].shape[0]):
        out['J%d' % s] = plane_error(got_J[s], ref['J'][s], ref['domain'], 'J[%d]' % s)
    return out


def report(tag, name, V_frac, spectral_index, errs):
    print('\n[gr factors, %s] case %-4s V_frac %-4g index %-3g ' % (tag, name, V_frac, spectral_index)
          + '  '.join('%s %.1e' % (k, e) for k, e in errs.items()))
