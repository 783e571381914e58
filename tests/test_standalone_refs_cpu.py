"""CPU half of the stand-alone kernel suite (tests/standalone_cases.py, tests/test_gpu_standalone_kernels.py):

 1. the float64 references the GPU cases are held to agree with each other, with scipy and with the goldens (1e-12);
 2. every case can see the slips it is for: the same inputs go through the reference and through a mutated reference,
    and the case's own comparator and bound must flag the mutant by at least 5x the bound (the convention of
    tests/test_gpu_bf16_faithful.py).  A case whose inputs hide its mutant fails here, before any GPU time is spent.
"""
import functools

import numpy as np
import pytest
import torch

import standalone_cases as sc
from oracle import oracle_np as onp
from oracle import oracle_torch as ot

MUTANT_FACTOR = 5.0


@functools.lru_cache(maxsize=4)
def prepared(case_id):
    case = next(c for c in sc.CASES if c.id == case_id)
    inp = sc.inputs(case)
    ref = sc.reference(case, inp)
    return case, inp, ref, sc.scales(case, inp, ref)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), np.abs(a - b).max() / np.abs(b).max()


# ---------------------------------------------------------------------------------------------------------------
# the table itself
# ---------------------------------------------------------------------------------------------------------------
def test_table_is_well_formed_and_covers_every_kernel():
    ids = [c.id for c in sc.CASES]
    assert len(set(ids)) == len(ids)
    assert set(sc.BY_FAMILY) == {'geom', 'rt', 'chi2', 'adam', 'eht', 'trilinear', 'voxel', 'grid'}
    for c in sc.CASES:
        assert len(c.why) > 10 and c.mutants, c                     # every case names its branch and carries at least one slip
        assert all(m in sc.MUTANTS for m in c.mutants), c
    used = {m for c in sc.CASES for m in c.mutants}
    assert used == set(sc.MUTANTS), set(sc.MUTANTS) - used          # every listed slip is assigned to a case that can show it


def test_eht_split_rule_gives_each_case_its_intended_RS():
    assert sc.eht_splits(1, 4097) == 2 and sc.eht_splits(3, 131073) == 64 and sc.eht_splits(42, 6145) == 3
    assert sc.eht_splits(21, 65536) == 32 and sc.eht_splits(7, 16) == 1
    for c in sc.BY_FAMILY['eht']:
        p = c.p
        assert sc.eht_splits(p['N'] * p['C'] * p['nvis'], p['R']) == p['RS'], c
    assert sc.eht_span(4097, 2) == 2050 and sc.eht_span(4098, 2) == 2050 and sc.eht_span(6145, 3) == 2050
    odd = [c for c in sc.BY_FAMILY['eht'] if c.p['RS'] > 1 and c.p['R'] % 2]
    assert {c.p['RS'] for c in odd} >= {2, 3, 64}
    # the slice marks are where the inputs say: a bright pixel on both sides of every slice boundary and at the end
    for c in odd:
        img = sc.inputs(c)['images']
        span = sc.eht_span(c.p['R'], c.p['RS'])
        assert img[0, span] > 10 * np.median(img[0]) and img[0, span - 1] > 10 * np.median(img[0]) and img[0, -1] > 10 * np.median(img[0])


# ---------------------------------------------------------------------------------------------------------------
# 1. references against each other, scipy and the goldens
# ---------------------------------------------------------------------------------------------------------------
def _autograd_eht(images, A, target, sigma, scale, dtype):          # tests/eht_uv_cases.py::dense_ref_loss
    img = torch.tensor(images, dtype=torch.float64, requires_grad=True)
    At, tg, sg = torch.tensor(A).to(torch.complex128), torch.tensor(target), torch.tensor(sigma)
    vec = img.reshape(img.shape[0], -1, 1).to(torch.complex128)
    if dtype == 'cphase':
        vis = (At @ vec[:, None]).squeeze(-1)
        loss = scale * ((1.0 - torch.cos(tg - torch.angle(vis.prod(dim=-2)))) / sg ** 2).sum()
    else:
        vis = (At @ vec).squeeze(-1)
        loss = scale * (((vis - tg).abs() / sg) ** 2).sum() if dtype == 'vis' else scale * (((vis.abs() - tg) / sg).abs() ** 2).sum()
    loss.backward()
    return loss.item(), img.grad.numpy()


@pytest.mark.parametrize('name', ['vis_odd_rs2', 'vis_below_rs2', 'amp_even_A8', 'cphase_odd_rs3', 'cphase_C8', 'cphase_C1', 'vis_300_terms'])
def test_eht_reference_equals_complex_autograd_and_the_oracle(name):
    case, inp, ref, _ = prepared('eht-' + name)
    p = case.p
    A = inp['A'].astype(np.complex128)
    A_l = A if p['dtype'] == 'cphase' else A[:, 0]
    tgt = inp['target'].astype(np.complex128 if p['dtype'] == 'vis' else np.float64)
    sig, scale = inp['sigma'].astype(np.float64), sc.r32(inp['scale'])
    loss, grad = _autograd_eht(inp['images'].astype(np.float64), A_l, tgt, sig, scale, p['dtype'])
    assert abs(float(ref['loss0']) - loss) <= 1e-12 * abs(loss)
    close(ref['dimg'], grad, 1e-11)
    R = p['R']
    want = onp.loss_eht(inp['images'].astype(np.float64).reshape(p['N'], 1, R), tgt, sig, A_l, scale, p['dtype'])
    assert abs(float(ref['loss0']) - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize('dtype', ['vis', 'amp', 'cphase'])
def test_eht_reference_on_the_golden(golden, dtype):
    g = golden('g7_eht')
    A = (g['A3'] if dtype == 'cphase' else g['A'][:, None]).astype(np.complex64)
    case = sc.Case('eht', 'golden', 'golden', (), dtype=dtype, N=3, C=A.shape[1], nvis=7, R=16, RS=1)
    tgt = g['target_' + dtype]
    inp = dict(images=g['images'].reshape(3, 16).astype(np.float32), A=A, target=tgt.astype(np.complex64 if dtype == 'vis' else np.float32),
               sigma=g['sigma'].astype(np.float32), scale=float(g['scale']))
    ref = sc.reference(case, inp)
    assert abs(float(ref['loss0']) - float(g['loss_' + dtype])) < 2e-6 * abs(float(g['loss_' + dtype]))       # float32-rounded inputs


def test_trilinear_reference_equals_scipy_and_the_cubic_oracle(golden):
    from scipy import ndimage
    for name in ('noncubic_gridstride', 'axis_1_and_2', 'misaligned'):
        case, inp, ref, _ = prepared('trilinear-' + name)
        grid, ext, pts = inp['grid'].astype(np.float64), inp['ext'].astype(np.float64), inp['points'].astype(np.float64)[:60000]
        index = np.stack([onp.world_to_index(pts[:, i], ext[i], grid.shape[i]) for i in range(3)])
        want = ndimage.map_coordinates(grid, index, order=1, mode='constant', cval=0.0)
        close(ref['out'][:len(pts)], want)
        assert (want == 0).any() and (want > 0).any()
        hit = sc._on_upper_face(pts.T, ext, grid.shape)
        assert hit.sum() >= 10 and (ref['out'][:len(pts)][hit] > 0).all()            # upper faces are inside (scipy agrees above)
    g = golden('g8_dynamics')
    fov = float(g['axis'][-1] - g['axis'][0])
    close(onp.trilinear_world(g['volume'], (fov,) * 3, *g['points'].T), g['interp'])
    rng = np.random.default_rng(0)
    per_frame = rng.uniform(size=(3, 4, 5, 6))
    u = rng.uniform(-1.2, 1.2, (3, 3, 50))
    got = onp.trilinear_world(per_frame, (2.0, 2.0, 2.0), *u)
    for b in range(3):
        idx = np.stack([onp.world_to_index(u[i, b], 2.0, per_frame.shape[1 + i]) for i in range(3)])
        close(got[b], ndimage.map_coordinates(per_frame[b], idx, order=1, mode='constant', cval=0.0))


def test_voxel_reference_equals_image_plane_dynamics_and_its_golden(golden):
    g = golden('g8_dynamics')
    fov = float(g['axis'][-1] - g['axis'][0])
    R, G = 20, 12
    flat = lambda v: np.asarray(v, dtype=np.float64).reshape(-1)
    tM0 = (g['t_frames'] - g['t_frames'][0]) / onp.GM_C3_SGRA_HR - float(g['t_injection'])
    w1 = flat(g['dtau'] * g['Sigma'])[None]
    geo = [flat(g['coords'][0]), flat(g['coords'][1]), flat(g['coords'][2]), flat(g['Omega']), flat(g['t_geos'])]
    img, _ = onp.voxel_render(g['volume'], (fov,) * 3, *geo, tM0, w1, R, G)
    close(img[:, 0].reshape(g['images'].shape), g['images'], 1e-11)
    wJ = (g['J'] * g['dtau'] * g['Sigma']).reshape(3, -1)
    imgJ, _ = onp.voxel_render(g['volume'], (fov,) * 3, *geo, tM0, wJ, R, G)
    close(imgJ.reshape(g['images_J'].shape), g['images_J'], 1e-11)
    # a grid per frame: frame b scaled by (1 + b) scales image b (trilinear sampling is linear in the grid)
    movie = np.stack([g['volume'] * (1.0 + b) for b in range(3)])
    img4, _ = onp.voxel_render(movie, (fov,) * 3, *geo, tM0, w1, R, G)
    close(img4[:, 0].reshape(g['images'].shape), g['images'] * np.array([1.0, 2.0, 3.0])[:, None, None], 1e-11)
    # three extents and sizes against the cubic composition on a resampled problem: scaling axis y of grid and points alike changes nothing
    geo2 = list(geo); geo2[2] = geo[2] * 1.5
    a, _ = onp.voxel_render(g['volume'], (fov, fov, 1.5 * fov), *geo2, tM0, w1, R, G)
    close(a, img, 1e-11)


def test_grid_reference_equals_the_oracle_the_golden_and_autograd(golden):
    g = golden('g9_grid')
    scale, rmin, rmax, zw, res = g['hparams']
    R, G = 20, 10
    flat = lambda v: np.asarray(v, dtype=np.float64).reshape(-1)
    c = g['coords']
    r2 = (c ** 2).sum(0)
    dom = flat(~((r2 < rmin ** 2) | (r2 > rmax ** 2) | (np.abs(c[2]) > zw))).astype(np.uint8)
    tM0 = g['t_frames'] / onp.GM_C3_SGRA_HR - float(g['t_injection'])
    geo = [flat(c[0]), flat(c[1]), flat(c[2]), flat(g['Omega']), flat(g['t_geos'])]
    e, _ = onp.grid_emission(g['grid'], scale, *geo, tM0, dom)
    close(e.reshape(g['emission'].shape), g['emission'], 1e-11)
    want = onp.grid_predictor_apply(g['grid'], g['t_frames'], c, g['Omega'], 0.0, g['t_geos'], float(g['t_injection']), scale=scale, rmin=rmin, rmax=rmax, z_width=zw)
    close(e.reshape(want.shape), want)
    w = flat(g['g'] ** 2 * g['dtau'] * g['Sigma'])[None]
    img = onp.render_weighted(e, w, R, G)
    close(img[:, 0].reshape(g['images'].shape), g['images'], 1e-11)
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64))
    geom = dict(coords=t(c), Omega=t(g['Omega']), t_geos=t(g['t_geos']), g=t(g['g']), dtau=t(g['dtau']), Sigma=t(g['Sigma']), t_start_obs=0.0, t_injection=float(g['t_injection']))
    hp = dict(GM_c3=onp.GM_C3_SGRA_HR, scale=float(scale), rmin=float(rmin), rmax=float(rmax), z_width=float(zw))
    _, _, gref = ot.grid_loss_and_grad(g['grid'], t(g['t_frames']), geom, hp, t(g['target']), t(g['sigma']))
    dimg = 2.0 * (img[:, 0] - g['target'].reshape(3, R)) / g['sigma'].reshape(3, R) ** 2
    grad = onp.grid_render_grad(g['grid'], scale, *geo, tM0, dom, w, dimg[:, None], R, G)
    close(grad, gref.numpy(), 1e-11)
    # polarised: linear in (w_s, dI_s) -- the sum of the unpolarised gradients -- and equal to central differences of the render
    rng = np.random.default_rng(1)
    w3, dI3 = rng.uniform(-1, 1, (3, R * G)), rng.normal(size=(3, 3, R))
    g3 = onp.grid_render_grad(g['grid'], scale, *geo, tM0, dom, w3, dI3, R, G)
    close(g3, sum(onp.grid_render_grad(g['grid'], scale, *geo, tM0, dom, w3[s:s + 1], dI3[:, s:s + 1], R, G) for s in range(3)))
    f = lambda gr: float((onp.render_weighted(onp.grid_emission(gr, scale, *geo, tM0, dom)[0], w3, R, G) * dI3).sum())
    for i, j, k in g['fd_idx'][:6]:
        d = np.zeros_like(g['grid']); d[i, j, k] = 1e-4
        assert abs((f(g['grid'] + d) - f(g['grid'] - d)) / 2e-4 - g3[i, j, k]) <= 1e-6 * np.abs(g3).max()


def test_simple_references_equal_the_oracle():
    for cid in ('adam-large_t', 'adam-t1_n255'):
        case, inp, ref, _ = prepared(cid)
        lr, b1, b2, eps, gs = (sc.r32(inp[k]) for k in ('lr', 'b1', 'b2', 'eps', 'gs'))
        t = inp['t']
        g, m0, v0 = inp['g'].astype(np.float64) * gs, inp['m'].astype(np.float64), inp['v'].astype(np.float64)
        m = b1 * m0 + (1 - b1) * g                                   # the three-line restatement
        v = b2 * v0 + (1 - b2) * g * g
        p = inp['p'] - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
        close(ref['m'], m); close(ref['v'], v)
        close(ref['p'], p, 1e-9)                                    # the library rounds 1 - b^t to float: 6e-8 of an update of 1e-2
        po, mo, vo = onp.adam_step(inp['p'].astype(np.float64), g, m0, v0, t, lr, b1, b2, eps)
        close(po, p); close(mo, m); close(vo, v)
    for cid in ('chi2-full_scalar_multitrip', 'chi2-lc_300_planes', 'chi2-lc_cancel'):
        case, inp, ref, _ = prepared(cid)
        a = {k: inp[k].astype(np.float64) for k in ('images', 'target', 'sigma', 'offset')}
        want = onp.loss_image(a['images'][..., None], a['target'], a['sigma'], a['offset'], sc.r32(inp['scale']), case.p['dtype']) if case.p['dtype'] == 'lc' \
            else onp.loss_image(a['images'], a['target'], a['sigma'], a['offset'], sc.r32(inp['scale']), 'full')
        assert abs(float(ref['loss0']) - want) <= 1e-12 * want and abs(ref['loss_planes'].sum() - want) <= 1e-12 * want
    case, inp, ref, _ = prepared('rt-lpr4_g13')
    close(ref['img'], onp.radiative_trasfer(*(inp[k].astype(np.float64) for k in ('e', 'g', 'dtau', 'Sigma'))))


def test_input_properties_the_cases_rely_on():
    # light curves that cancel: sum|pixels| / |sum pixels| >= 1e4, so a float accumulation cannot meet the result-relative bound
    for cid in ('chi2-lc_cancel', 'chi2-lc_cancel_scalar'):
        img = sc.inputs(next(c for c in sc.CASES if c.id == cid))['images'].astype(np.float64)
        assert (np.abs(img).sum(-1) / np.abs(img.sum(-1))).min() >= 1e4
    # boundary-equality cases: r^2 is exact in float32 (the kernel's own order of operations) and each boundary is hit
    for c in sc.BY_FAMILY['geom']:
        inp = sc.inputs(c)
        x, y, z = inp['coords']
        r2_32 = (x * x + y * y) + z * z
        r2 = (inp['coords'].astype(np.float64) ** 2).sum(0)
        assert r2_32.dtype == np.float32
        if c.p['exact']:
            assert np.array_equal(r2_32.astype(np.float64), r2)
            if c.p['P'] > 1:
                assert (r2 == 9).sum() >= 3 and (r2 == 81).sum() >= 3 and ((np.abs(z) == 8) & (r2 <= 81)).sum() >= 3
        else:
            for v, b in ((r2, 9.0), (r2, 81.0), (np.abs(z).astype(np.float64), 8.0)):       # no tie: nothing is excluded
                assert np.abs(v - b).min() > 16 * 2.0 ** -23 * b
            assert ((r2_32 < 9) | (r2_32 > 81) | (np.abs(z) > 8)).tolist() == ((r2 < 9) | (r2 > 81) | (np.abs(z) > 8)).tolist()
    # samplers: every index is exactly on a face or clear of it by far more than float32 rounding; t_M is clear of 0
    for c in sc.BY_FAMILY['voxel'] + sc.BY_FAMILY['grid'] + sc.BY_FAMILY['trilinear']:
        inp = sc.inputs(c)
        if c.family == 'trilinear':
            us, exts, ns = inp['points'].astype(np.float64).T, inp['ext'], inp['grid'].shape
        else:
            ux, uy, uz, _ = onp.warp_points(inp['x'], inp['y'], inp['z'], inp['Omega'], inp['t_geo'], inp['tM0'])
            us = (ux, uy, uz)
            exts, ns = (inp['ext'], inp['grid'].shape[-3:]) if c.family == 'voxel' else ((2 * inp['scale'],) * 3, inp['grid'].shape)
            tM = inp['tM0'][:, None] + inp['t_geo'].astype(np.float64)[None]
            assert np.abs(tM).min() > 1e-2 and (tM < 0).any() and (tM > 0).any()
        faces = 0
        for u, f, n in zip(us, exts, ns):
            i = onp.world_to_index(u, float(f), n)
            for edge in (0.0, n - 1.0):
                dist = np.abs(i - edge)
                assert ((dist == 0) | (dist > 1e-4 * max(n - 1, 1))).all() or n == 1, (c, edge)
                faces += int((dist == 0).sum())
        assert faces > 0, c                                           # every sampler case has samples exactly on a face


# ---------------------------------------------------------------------------------------------------------------
# 2. the cases can see the errors they are for
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id,mutant', [(c.id, m) for c in sc.CASES for m in c.mutants])
def test_case_flags_its_mutant_by_5x_its_bound(case_id, mutant):
    case, inp, ref, scl = prepared(case_id)
    assert sc.worst(sc.errors(case, ref, ref, scl)) == 0.0
    bad = sc.reference(case, inp, mutant)
    errs = sc.errors(case, bad, ref, scl)
    assert sc.worst(errs) >= MUTANT_FACTOR, sc.report(case, errs)


@pytest.mark.parametrize('case_id', [c.id for c in sc.CASES])
def test_case_inputs_are_deterministic_and_float32(case_id):
    case = next(c for c in sc.CASES if c.id == case_id)
    a, b = sc.inputs(case), sc.inputs(case)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=False), k
        if isinstance(a[k], np.ndarray) and k not in ('tM0', 'dom', 'A'):
            assert a[k].dtype == np.float32 or (k == 'target' and a[k].dtype == np.complex64), (k, a[k].dtype)
