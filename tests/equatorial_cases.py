"""What the CPU and the GPU tests of the equatorial crossings (geodesics.equatorial_crossings, bhn_eql_crossings) share: the ray sets,
the host back end's answers (computed once per case and left unchanged) and the closed forms of Gralla & Lupsasca 2020 the
crossings are held to.  Imported by the tests the way gr_factor_cases.py is."""
import numpy as np

from bhnerf_amd import geodesics as G

GR_TOL = 1e-10
ROWS = ('mino', 'r', 'theta', 'phi', 't', 'vr', 'vth')
H, R_C, MAX_STEPS, NMAX = 0.02, 5.0, 400000, 3
FOV = (-9.0, 9.0)

# the 70-ray grid (10 x 7 over (-9, 9)^2: one wave and a 6-lane tail) of the tracer's tests: name -> (spin, inclination)
GRID_CASES = {'spin 0.94 / 60 deg': (0.94, np.deg2rad(60.0)), 'spin 0.94 / 17 deg': (0.94, np.deg2rad(17.0)),
              'spin 0 / 60 deg': (0.0, np.deg2rad(60.0))}
# the 12 rays (3 x 4 over (-9, 9)^2) of the closed-form tests of tests/test_geodesics_cpu.py, all with eta > 1: (spin, inclination)
CLOSED_FORM_CASES = [(0.94, np.deg2rad(60.0)), (0.0, np.deg2rad(60.0))]


def grid_rays(num_alpha=10, num_beta=7):
    alpha, beta = np.meshgrid(np.linspace(*FOV, num_alpha), np.linspace(*FOV, num_beta), indexing='ij')
    return alpha.ravel(), np.where(beta == 0.0, 1e-9, beta).ravel()


_HOST = {}


def host_crossings(spin, inc, num_alpha=10, num_beta=7):
    """(cross (7, n, NMAX) of the forward equations, count, lam, eta) of the NumPy back end on a grid, computed once."""
    key = (spin, inc, num_alpha, num_beta)
    if key not in _HOST:
        alpha, beta = grid_rays(num_alpha, num_beta)
        _HOST[key] = G._integrate_crossings(alpha, beta, spin, inc, 1000.0, 1.0, H, R_C, MAX_STEPS, NMAX)
    return _HOST[key]


def host_ends(spin, inc):
    """(mino_end, state_end) of the host tracer on the 70-ray grid, computed once."""
    key = ('end', spin, inc)
    if key not in _HOST:
        _HOST[key] = G.trace(*grid_rays(), spin, inc)[:2]
    return _HOST[key]


def row_errors(got, want):
    """Per row: max |got - want| over the finite elements / the row's largest magnitude; the NaN patterns must be equal."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return np.array([np.abs(g[f] - w[f]).max() / max(np.abs(w[f]).max(), 1e-300) if f.any() else 0.0 for g, w, f in zip(got, want, fin)])


def closed_form_crossing_times(spin, inc, lam, eta, beta, count):
    """Mino times (elapsed since the observer) of the first `count` zeros of cos theta(tau) of Gralla & Lupsasca 2020, eq. 38,
        cos theta = -nu sqrt(u_+) sn(w (tau + nu G_o) | m):   tau_j = 2 j K(m) / w - nu G_o,   j = 0, 1, ... (those with tau > 0),
    w = sqrt(-u_- a^2), m = u_+ / u_-, and its a -> 0 form (sin, w = sqrt(eta + lam^2), K = pi / 2).  mpmath, 30 digits; the code
    pattern of tests/test_geodesics_cpu.py."""
    import mpmath as mp
    mp.mp.dps = 30
    lam, eta, a, th_o = mp.mpf(float(lam)), mp.mpf(float(eta)), mp.mpf(spin), mp.mpf(float(inc))
    assert eta > 0
    nu = -1 if beta > 0 else 1
    if a == 0:
        up, w = eta / (eta + lam ** 2), mp.sqrt(eta + lam ** 2)
        G_o, K = -mp.asin(mp.cos(th_o) / mp.sqrt(up)) / w, mp.pi / 2
    else:
        D = (1 - (eta + lam ** 2) / a ** 2) / 2
        up, um = D + mp.sqrt(D ** 2 + eta / a ** 2), D - mp.sqrt(D ** 2 + eta / a ** 2)
        w, m = mp.sqrt(-um * a ** 2), up / um
        G_o, K = -mp.re(mp.ellipf(mp.asin(mp.cos(th_o) / mp.sqrt(up)), m)) / w, mp.re(mp.ellipk(m))
    out, j = [], 0
    while len(out) < count:
        tau = 2 * j * K / w - nu * G_o
        if tau > 0:
            out.append(tau)
        j += 1
    return out


def gl_radial_integral(r, roots):
    """I_r(r) = int_{r4}^{r} dr / sqrt(R(r)) for four real roots r1 < r2 < r3 < r4 <= r (Gralla & Lupsasca 2020, eq. B35 / B40)."""
    import mpmath as mp
    r1, r2, r3, r4 = roots
    r31, r32, r41, r42 = r3 - r1, r3 - r2, r4 - r1, r4 - r2
    k = r32 * r41 / (r31 * r42)
    x2 = (r - r4) * r31 / ((r - r3) * r41)
    return 2 / mp.sqrt(r31 * r42) * mp.ellipf(mp.asin(mp.sqrt(x2)), k)


def closed_form_errors(spin, inc, cross, count, lam, eta, beta, distance=1000.0):
    """The crossings (7, n, nmax) of n rays with eta > 1 against the closed forms: (polar, radial, rays in the radial check,
    crossings in it).  polar: largest |mino - tau_j| sqrt(eta) over every crossing found (to be <= 1e-9: the project's polar bound,
    1e-9 in cos theta, carried through the slope of cos theta at the equator, sqrt(eta)); radial: on the scattering rays with four
    real roots, largest |mino - (I_r(r_o) -+ I_r(r_cross))| over the ray's total Mino time 2 I_r(r_o) (before / after the radial
    turning point: the sign of v_r at the crossing)."""
    import mpmath as mp
    mp.mp.dps = 30
    polar, radial, n_rays, n_cross = 0.0, 0.0, 0, 0
    for i in range(len(count)):
        assert eta[i] > 1.0
        taus = closed_form_crossing_times(spin, inc, lam[i], eta[i], beta[i], int(count[i]))
        for j, tau in enumerate(taus):
            polar = max(polar, abs(float(tau - mp.mpf(float(cross[0, i, j])))) * np.sqrt(eta[i]))
        a, l, e = spin, float(lam[i]), float(eta[i])
        roots = mp.polyroots([1, 0, a * a - e - l * l, 2 * (e + (l - a) ** 2), -a * a * e], maxsteps=200, extraprec=200)
        if count[i] == 0 or any(abs(mp.im(z)) > 1e-12 for z in roots):
            continue                                           # plunging ray: two complex roots, another case of the paper
        roots = sorted(mp.re(z) for z in roots)
        if np.nanmin(cross[1, i]) < float(roots[3]):
            continue                                           # a ray inside the turning radius: captured
        I_o = gl_radial_integral(mp.mpf(distance), roots)
        for j in range(int(count[i])):
            I_x = gl_radial_integral(mp.mpf(float(cross[1, i, j])), roots)
            want = I_o - I_x if cross[5, i, j] < 0 else I_o + I_x
            radial = max(radial, abs(float(want - mp.mpf(float(cross[0, i, j])))) / float(2 * I_o))
            n_cross += 1
        n_rays += 1
    return polar, radial, n_rays, n_cross
