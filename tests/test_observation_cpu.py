"""Host tests of the observation layer between a station table and the EHT operators: observation.Array, empty_eht_obs,
Observation.add_thermal_noise, Observation.closure_sets and Observation.data.  NumPy float64, no GPU.

The two station tables under tests/golden/eht_arrays/ are the reference's data files, unchanged.  Fixture g11 (made by
tests/golden/make_eht2017.py from the same EHT2017 table) pins the closed form; a second formulation written here (rotate the
stations by GMST about z, project on the east and north unit vectors of the source) is independent of it."""
import os

import numpy as np
import pytest

from bhnerf_amd import observation

ARRAYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eht_arrays')


@pytest.fixture(scope='module')
def eht2017():
    return observation.Array.load_txt(os.path.join(ARRAYS, 'EHT2017.txt'))


@pytest.fixture(scope='module')
def ngeht():
    return observation.Array.load_txt(os.path.join(ARRAYS, 'ngEHT.txt'))


@pytest.fixture(scope='module')
def track(eht2017):
    """EHT2017 on Sgr A*, 12 frames from GMST 19 h to 24 h (both ends a frame), default elevation limits: the station set changes
    along it."""
    return observation.empty_eht_obs(eht2017, 12, 60.0, timetype='GMST', times=np.linspace(19.0, 24.0, 12))


@pytest.fixture(scope='module')
def ngeht_obs(ngeht):
    """Tutorial 4's observation: ngEHT, GMST 2 h + 40 min, 64 frames, 30 s scans."""
    return observation.empty_eht_obs(ngeht, 64, 30.0, tstart=2.0, tstop=2.0 + 40.0 / 60.0, mjd=57851, timetype='GMST')


TRACK_STATIONS_UP = [4, 4, 5, 5, 5, 4, 5, 5, 5, 5, 5, 7]


def test_both_table_formats_parse(eht2017, ngeht, golden):
    assert len(ngeht) == 23 and ngeht.pairs.shape == (253, 2) and ngeht.xyz.shape == (23, 3)
    assert ngeht.names[0] == 'ALMA' and ngeht.names[-1] == 'PV' and ngeht.sefd[0] == 70.0 and ngeht.sefd[9] == 10000.0     # 5 columns: SEFDL = SEFDR
    g = golden('g11_eht2017')
    assert len(eht2017) == 8 and eht2017.names == [str(s) for s in g['sites']]
    assert np.array_equal(eht2017.xyz, g['xyz']) and np.array_equal(eht2017.sefd, g['sefd'])
    assert eht2017.sefd[2] == 0.5 * (5600 + 6500)                                  # SMA: the one station whose SEFDR and SEFDL differ
    assert np.array_equal(eht2017.pairs, g['pairs'])
    assert (eht2017.pairs[:, 0] < eht2017.pairs[:, 1]).all()
    with pytest.raises(AttributeError):
        observation.Array(['A', 'B'], np.zeros((2, 3)), [1.0])
    with pytest.raises(AttributeError):
        observation.empty_eht_obs('EHT2017', 4, 60.0)


def test_g11_is_reproduced(eht2017, golden):
    g = golden('g11_eht2017')
    # the three lines of tests/golden/make_eht2017.py that place the track in sidereal time
    ra = (17 + 45 / 60 + 40.0409 / 3600) * 15.0 * np.pi / 180
    gst0 = ra + np.deg2rad(110.0) - 4.0 / 24 * 2 * np.pi
    gst = gst0 + g['t_hr'] / 23.9344696 * 2 * np.pi
    obs = observation.empty_eht_obs(eht2017, 64, 60.0, ra=17 + 45 / 60 + 40.0409 / 3600, dec=-(29 + 0 / 60 + 28.118 / 3600), rf=230e9, bw=4e9,
                                    timetype='GMST', times=gst * 12.0 / np.pi, elev_max=90.0)
    assert obs.uv.shape == (64, 28, 2) and obs.uv.dtype == np.float64 and obs.up.dtype == bool
    assert obs.sigma.shape == obs.up.shape == (64, 28) and obs.elevation.shape == (64, 8) and obs.times.shape == obs.gmst.shape == (64,)
    err = np.abs(obs.uv - g['uv']).max() / np.abs(g['uv']).max()
    print('\n[observation] g11: uv %.1e of max |uv|, sigma %.1e relative' % (err, np.abs(obs.sigma / g['sigma'] - 1).max()))
    assert err <= 1e-9
    assert np.array_equal(obs.up, g['up']) and 0 < obs.up.sum() < obs.up.size
    assert np.abs(obs.sigma / g['sigma'] - 1).max() <= 1e-12
    assert (obs.ra, obs.rf, obs.bw, obs.tint) == (17 + 45 / 60 + 40.0409 / 3600, 230e9, 4e9, 60.0)


def _rotated(array, obs):
    """(u, v, w) in wavelengths another way: the stations' positions rotated by GMST about z into the celestial frame, projected
    on the east, north and source unit vectors of (ra, dec)."""
    a, d = obs.ra * np.pi / 12.0, np.deg2rad(obs.dec)
    east = np.array([-np.sin(a), np.cos(a), 0.0])
    north = np.array([-np.sin(d) * np.cos(a), -np.sin(d) * np.sin(a), np.cos(d)])
    src = np.array([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)])
    th = obs.gmst * np.pi / 12.0
    c, s, z = np.cos(th), np.sin(th), np.zeros_like(th)
    R = np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, z + 1], -1)], -2)         # (nt, 3, 3)
    pos = np.einsum('tij,nj->tni', R, array.xyz)
    B = (pos[:, obs.pairs[:, 1]] - pos[:, obs.pairs[:, 0]]) / (observation.C_LIGHT / obs.rf)
    return B @ east, B @ north, B @ src, pos @ src / np.linalg.norm(array.xyz, axis=1)


@pytest.mark.parametrize('which', ['eht2017', 'ngeht'])
def test_closed_form_against_an_independent_formulation(which, request):
    array = request.getfixturevalue(which)
    obs = observation.empty_eht_obs(array, 16, 30.0, tstart=1.0, tstop=23.0, mjd=57851)             # a UTC day
    assert obs.timetype == 'UTC' and np.array_equal(obs.times, 1.0 + np.arange(16) * (22.0 / 16))
    u, v, w, sin_el = _rotated(array, obs)
    scale = np.abs(obs.uv).max()
    err = max(np.abs(obs.uv[..., 0] - u).max(), np.abs(obs.uv[..., 1] - v).max()) / scale
    B = array.xyz[obs.pairs[:, 1]] - array.xyz[obs.pairs[:, 0]]
    length = np.abs((obs.uv ** 2).sum(-1) + w ** 2 - (B ** 2).sum(-1) / (observation.C_LIGHT / obs.rf) ** 2).max() / scale ** 2
    print('\n[observation] %s: closed form against rotation %.1e of max |uv|, |uv|^2 + w^2 against |B|^2 %.1e' % (which, err, length))
    assert err <= 1e-12 and length <= 1e-12
    assert np.abs(np.sin(obs.elevation) - sin_el).max() <= 1e-12
    lo, hi = np.deg2rad(10.0), np.deg2rad(85.0)
    site_up = (obs.elevation > lo) & (obs.elevation < hi)
    assert np.array_equal(obs.up, site_up[:, obs.pairs[:, 0]] & site_up[:, obs.pairs[:, 1]])
    want = np.sqrt(array.sefd[obs.pairs[:, 0]] * array.sefd[obs.pairs[:, 1]] / (2 * 1856000000.0 * 30.0)) / 0.88
    assert np.abs(obs.sigma / want - 1).max() <= 1e-12


def test_utc_to_gmst():
    wrap = lambda h: (h + 12.0) % 24.0 - 12.0
    assert abs(wrap(observation.utc_to_gmst(51544, 12.0) - 18.697374558)) <= 1e-6            # JD 2451545.0 is MJD 51544.5
    assert abs(wrap(observation.utc_to_gmst(51544, 12.0 + 24.0 * 0.99726956633) - 18.697374558)) <= 1e-6      # one sidereal day on
    assert abs(wrap(observation.utc_to_gmst(57850, 4.0) - observation.utc_to_gmst(57850 + 0.99726956633, 4.0))) <= 1e-6
    obs = observation.empty_eht_obs(observation.Array(['A', 'B'], [[6e6, 0, 0], [0, 6e6, 0]], [1e3, 1e3]), 3, 10.0, tstart=0.0, tstop=3.0)
    assert np.allclose(obs.gmst, observation.utc_to_gmst(57850, np.array([0.0, 1.0, 2.0])), rtol=0, atol=1e-12)


def _rank(rows):
    return 0 if len(rows) == 0 else int(np.linalg.matrix_rank(np.asarray(rows, dtype=np.float64)))


def _design(obs, f, triangles, quadrangles):
    """The +-1 design matrices of the closure phases / log closure amplitudes over the baselines that frame f observes."""
    col = {tuple(p): i for i, p in enumerate(obs.pairs[obs.up[f]].tolist())}
    tri_rows = np.zeros((len(triangles), len(col)))
    for r, (a, b, c) in enumerate(triangles):
        tri_rows[r, col[(a, b)]] += 1; tri_rows[r, col[(b, c)]] += 1; tri_rows[r, col[(a, c)]] -= 1
    quad_rows = np.zeros((len(quadrangles), len(col)))
    for r, legs in enumerate(quadrangles):
        for leg, p in enumerate(legs):
            quad_rows[r, col[tuple(p)]] += 1 if leg < 2 else -1
    return tri_rows, quad_rows


def test_closure_sets_follow_the_changing_coverage(track):
    obs = track
    m_up = [len(obs._stations_up(f)) for f in range(obs.nt)]
    assert m_up == TRACK_STATIONS_UP
    assert [int(n) for n in obs.up.sum(1)] == [m * (m - 1) // 2 for m in m_up]
    rows = {}
    for count in ('min', 'max'):
        tris, tri_obs, quads, quad_obs = obs.closure_sets(count)
        assert tris == sorted(set(tris)) and quads == sorted(set(quads))
        assert tri_obs.shape == (12, len(tris)) and quad_obs.shape == (12, len(quads))
        assert tri_obs.any(0).all() and quad_obs.any(0).all()                       # the union: every member is observed somewhere
        assert all(a < b < c for a, b, c in tris)
        forms = {tuple(map(tuple, q)) for q in observation.closure_quadrangles(8).tolist()}
        assert set(quads) <= forms                                                   # the two forms per quadruple that the package defines
        rows[count] = (tri_obs.sum(1), quad_obs.sum(1))
        for f, m in enumerate(m_up):
            ft = [t for t, o in zip(tris, tri_obs[f]) if o]
            fq = [q for q, o in zip(quads, quad_obs[f]) if o]
            tri_rows, quad_rows = _design(obs, f, ft, fq)                            # (KeyError if a leg were a baseline that is down)
            assert _rank(tri_rows) == (m - 1) * (m - 2) // 2 and _rank(quad_rows) == m * (m - 3) // 2, (count, f, m)
            if count == 'min':
                assert len(ft) == (m - 1) * (m - 2) // 2 and len(fq) == m * (m - 3) // 2, (f, m, len(ft), len(fq))
                ref = min(obs._stations_up(f), key=lambda s: (obs.array.sefd[s], s))
                assert all(ref in t for t in ft)
            else:
                assert len(ft) == m * (m - 1) * (m - 2) // 6 and len(fq) == 2 * (m * (m - 1) * (m - 2) * (m - 3) // 24)
    assert (rows['max'][0] >= rows['min'][0]).all() and (rows['max'][1] >= rows['min'][1]).all()
    assert rows['max'][0].sum() > rows['min'][0].sum() and rows['max'][1].sum() > rows['min'][1].sum()
    # the same call gives the same tables (the quadrangle sets are cached per set of up stations)
    again = obs.closure_sets('min')
    assert again[0] == obs.closure_sets('min')[0] and again[2] == obs.closure_sets('min')[2]


def _vis_of_point_sources(obs, seed=1):
    """Visibilities of three point sources: every baseline has an amplitude well off zero and every closure quantity a value."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-20e-6, 20e-6, (3, 2)) / 206265.0
    flux = np.array([1.0, 0.3, 0.2])
    return (flux * np.exp(-2j * np.pi * (obs.uv[..., 0:1] * xy[:, 0] + obs.uv[..., 1:2] * xy[:, 1]))).sum(-1)


@pytest.mark.parametrize('count', ['min', 'max'])
def test_unobserved_entries_carry_no_weight(track, count):
    obs = track
    vis = _vis_of_point_sources(obs)
    assert np.abs(vis).min() > 10 * obs.sigma.max()
    data = obs.data(vis, 'amp+cphase+logcamp', count=count)
    tris, tri_obs, quads, quad_obs = obs.closure_sets(count)
    assert data['triangles'] == tris and data['quadrangles'] == quads
    for term, observed in (('amp', obs.up), ('cphase', tri_obs), ('logcamp', quad_obs)):
        target, sigma = data[term]
        assert target.shape == sigma.shape == observed.shape and (~observed).any() and observed.any()
        assert np.isposinf(sigma[~observed]).all() and (target[~observed] == 0).all()
        assert np.isfinite(sigma[observed]).all() and (sigma[observed] > 0).all() and (target[observed] != 0).all()
        assert np.isfinite(target).all()
    t, s = obs.data(vis, 'vis')['vis']
    assert t.dtype == np.complex64 and np.isposinf(s[~obs.up]).all() and (t[~obs.up] == 0).all() and np.array_equal(s[obs.up], obs.sigma[obs.up])
    assert np.array_equal(t[obs.up], vis.astype(np.complex64)[obs.up])
    # the observed values are the closure quantities of the tables
    op = observation.ClosureDFT(obs.uv, 1.0, 1, pairs=obs.pairs, triangles=tris, quadrangles=quads)
    assert np.array_equal(data['cphase'][0][tri_obs], op.closure_phases(vis)[tri_obs])
    plain = obs.data(vis, 'amp+logcamp', count=count, debias=False)
    assert np.array_equal(plain['amp'][0][obs.up], np.abs(vis)[obs.up])
    assert np.array_equal(plain['logcamp'][0][quad_obs], op.log_closure_amplitudes(vis)[quad_obs])
    deb = np.sqrt(np.maximum(np.abs(vis) ** 2 - obs.sigma ** 2, 0.0))
    assert np.array_equal(data['amp'][0][obs.up], deb[obs.up])
    assert np.array_equal(data['logcamp'][0][quad_obs], op.log_closure_amplitudes(deb)[quad_obs])
    # a Stokes axis: the planes share the tables and the sigmas
    both = obs.data(np.stack([vis, 0.5 * vis], axis=1), 'cphase+logcamp', count=count)
    assert both['cphase'][0].shape == (12, 2, len(tris)) and np.array_equal(both['cphase'][0][:, 0], data['cphase'][0])
    assert np.array_equal(both['logcamp'][1][:, 0], data['logcamp'][1])
    with pytest.raises(AttributeError):
        obs.data(vis, 'logcamp+cphase')
    with pytest.raises(AttributeError):
        obs.data(vis, 'vis+amp')
    with pytest.raises(AttributeError):
        obs.data(vis[:, :5], 'vis')
    with pytest.raises(AttributeError):
        obs.data(vis, 'cphase', count='some')


def test_no_closure_quantity_at_all_is_an_error(eht2017):
    three = observation.Array(eht2017.names[:3], eht2017.xyz[:3], eht2017.sefd[:3])
    obs = observation.empty_eht_obs(three, 4, 60.0, tstart=19.0, tstop=24.0, timetype='GMST', elev_min=-91.0, elev_max=91.0)
    vis = _vis_of_point_sources(obs)
    assert len(obs.data(vis, 'cphase')['triangles']) == 1
    with pytest.raises(AttributeError):
        obs.data(vis, 'logcamp')                                        # three stations have no quadrangle
    down = observation.empty_eht_obs(three, 4, 60.0, tstart=19.0, tstop=24.0, timetype='GMST', elev_min=89.0, elev_max=90.0)
    assert not down.up.any()
    with pytest.raises(AttributeError):
        down.data(vis, 'cphase')


def test_thermal_noise(ngeht_obs):
    obs = ngeht_obs
    assert obs.up.sum() == 64 * 153 and (obs.up.sum(1) == 153).all()
    zero = np.zeros(obs.up.shape, dtype=np.complex64)
    n = obs.add_thermal_noise(zero, seed=7)
    assert n.dtype == np.complex64 and n.shape == zero.shape
    assert (n[~obs.up] == 0).all() and (n[obs.up] != 0).all()
    stat = (np.abs(n[obs.up].astype(np.complex128)) ** 2 / (2 * obs.sigma[obs.up] ** 2)).mean()
    print('\n[observation] mean |n|^2 / (2 sigma^2) over %d entries: %.4f' % (obs.up.sum(), stat))
    assert abs(stat - 1.0) <= 0.05                                      # 5 / sqrt(64 * 153)
    assert n.tobytes() == obs.add_thermal_noise(zero, seed=7).tobytes() and n.tobytes() != obs.add_thermal_noise(zero, seed=8).tobytes()
    # the documented draw: one standard_normal of vis.shape + (2,), real parts first
    draw = np.random.default_rng(7).standard_normal(zero.shape + (2,))
    want = np.where(obs.up, obs.sigma * (draw[..., 0] + 1j * draw[..., 1]), 0.0).astype(np.complex64)
    assert n.tobytes() == want.tobytes()
    stokes = obs.add_thermal_noise(np.zeros((64, 3, 253), dtype=np.complex64), seed=7)
    assert stokes.shape == (64, 3, 253) and (stokes[:, :, ~obs.up[0]][0] == 0).all()


def test_closure_sigmas_and_debiasing_against_noise_draws(eht2017):
    """4000 noise draws on four stations held at one instant: the spread of one closure phase and one log closure amplitude
    against the sigma that Observation.data quotes for the noise-free visibilities, and the debiased amplitudes."""
    ndraw = 4000
    four = observation.Array(eht2017.names[:4], eht2017.xyz[:4], eht2017.sefd[:4])
    obs = observation.empty_eht_obs(four, ndraw, 60.0, timetype='GMST', times=np.full(ndraw, 21.0), elev_min=-91.0, elev_max=91.0)
    assert obs.up.all() and obs.nvis == 6
    snr = np.array([20.0, 24.0, 30.0, 22.0, 40.0, 26.0])                              # per baseline, at least 20
    truth = np.broadcast_to(snr * obs.sigma[0] * np.exp(1j * np.array([0.3, -1.1, 2.0, 0.7, -2.5, 1.4])), (ndraw, 6))
    quoted = obs.data(truth, 'cphase+logcamp', debias=False)
    assert len(quoted['triangles']) == 3 and len(quoted['quadrangles']) == 2
    noisy = obs.add_thermal_noise(truth, seed=11).astype(np.complex128)
    drawn = obs.data(noisy, 'amp+cphase+logcamp')
    for term in ('cphase', 'logcamp'):
        formula = quoted[term][1][0, 0]
        resid = drawn[term][0][:, 0] - quoted[term][0][0, 0]
        if term == 'cphase':
            resid = np.angle(np.exp(1j * resid))
        got = resid.std()
        print('\n[observation] %s: empirical sigma %.5f, formula %.5f (%.1f %%)' % (term, got, formula, 100 * (got / formula - 1)))
        assert abs(got / formula - 1) <= 0.06
        want = np.sqrt((1.0 / snr[[0, 3, 1]] ** 2).sum()) if term == 'cphase' else None
        if want is not None:                                                           # triangle (0, 1, 2) of pairs 01, 12, 02
            assert quoted['triangles'][0] == (0, 1, 2) and abs(formula / want - 1) <= 1e-12
    amp2 = drawn['amp'][0] ** 2
    se = amp2.std(0) / np.sqrt(ndraw)
    assert (np.abs(amp2.mean(0) - np.abs(truth[0]) ** 2) <= 5 * se).all(), (amp2.mean(0), np.abs(truth[0]) ** 2, se)
    assert np.array_equal(drawn['amp'][0], np.sqrt(np.maximum(np.abs(noisy) ** 2 - obs.sigma ** 2, 0.0)))


def test_trainstep_eht_obs_routes_by_dtype(track):
    """The host side of TrainStep.eht_obs: a single 'vis', 'amp' or 'cphase' becomes the TrainStep.eht_uv step (a DirectDFT), 'logcamp'
    and '+'-joined sets the TrainStep.eht_closure step (a ClosureDFT, the terms packed in the canonical order)."""
    from bhnerf_amd import optimization, units
    obs = track
    vis = _vis_of_point_sources(obs)
    t_frames = np.linspace(0.0, 0.5, 12) * units.hr
    for dtype in ('vis', 'amp', 'cphase'):
        step = optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, dtype)
        target, sigma, op = step.args[0].host_args
        want_t, want_s = obs.data(vis, dtype)[dtype]
        assert step.num_losses == 1 and step.dtype[0] == dtype and type(op) is observation.DirectDFT and op.uv is not None
        assert np.array_equal(target, want_t.astype(target.dtype)) and np.array_equal(sigma, want_s.astype(np.float32))
        assert (op.ncp > 0) == (dtype == 'cphase') and np.isposinf(sigma).any() and np.array_equal(op.uv, obs.uv)
    for dtype, count in (('logcamp', 'min'), ('cphase+logcamp', 'max'), ('amp+cphase+logcamp', 'min')):
        step = optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, (16, 12), dtype, count=count, weights={'logcamp': 0.5})
        target, sigma, op = step.args[0].host_args
        data = obs.data(vis, dtype, count=count)
        assert step.dtype[0] == dtype and isinstance(op, observation.ClosureDFT) and op.weights['logcamp'] == 0.5 and (op.H, op.W) == (16, 12)
        parts = op.split(sigma, dtype)
        assert list(parts) == dtype.split('+')
        for term in parts:
            assert np.array_equal(parts[term], data[term][1].astype(np.float32))
            assert np.array_equal(op.split(target, dtype)[term], data[term][0].astype(np.float32))
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, 'amp', weights={'amp': 2.0})
    with pytest.raises(AttributeError):
        optimization.TrainStep.eht_obs(t_frames, obs, vis, 1e-10, 16, 'logcamp+vis')
