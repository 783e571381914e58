"""CPU half of the volume-render suite (tests/volume_cases.py, tests/test_gpu_volume.py):

 1. the float64 restatement the GPU cases are held to reproduces the images the reference's own visualization.py rendered
    (tests/golden/g13_volume.npz, written by tests/golden/make_volume.py) to 1e-12, and VolumeVisualizer.set_view reproduces the
    reference's points, step lengths and coords to 1e-12;
 2. VolumeVisualizer's argument handling, which needs no device;
 3. every case sees the slips it is for at >= 5x the bound, and the bound is not under the restatement's own float32 floor;
 4. the new entry point is declared, exported and bound.
"""
import functools
import os
import sys

import numpy as np
import pytest

import volume_cases as vc
from bhnerf_amd import _hip, visualization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def prepared(case_id):
    case = next(c for c in vc.CASES if c.id == case_id)
    inp = vc.inputs(case)
    wire = vc.wire_alpha(inp['pts'], inp['fw'], inp['lw'])
    return case, inp, wire, vc.reference(case, inp, wire=wire)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement and set_view against the reference's own output
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('view', ['a', 'b'])
def test_restatement_reproduces_the_reference_images(view):
    g = vc.golden()
    domain_r, cam_r, fw, lw, bh = g['params'][:5]
    albedo = g['params'][5:8]
    pts, e = g['pts_' + view].astype(np.float64), g['emission_' + view].astype(np.float64)[None]
    scale = np.array([1.0 / e.max()])
    wire = vc.wire_alpha(pts, fw, lw)
    close(vc.render_ref(pts, e, scale, g['lut_hot'], fw, lw, 0.0, (0, 0, 0), wire=wire)[0], g['image_%s_nobh' % view])
    close(vc.render_ref(pts, e, scale, g['lut_hot'], fw, lw, bh, albedo, wire=wire)[0], g['image_%s_bh' % view])
    assert np.abs(g['image_%s_bh' % view] - g['image_%s_nobh' % view]).max() > 0.1          # the black hole is in the picture
    assert g['image_%s_nobh' % view].max() > 3.0 and g['image_%s_nobh' % view].min() < 0.05   # emission inside the cube, and the wires


def test_set_view_reproduces_the_reference_points_steps_and_coords():
    g = vc.golden()
    domain_r, cam_r = g['params'][:2]
    for view in ('a', 'b'):
        W, H, S, az, zen = g['view_' + view]
        viz = visualization.VolumeVisualizer(int(W), int(H), int(S))
        assert viz.coords is None
        viz.set_view(cam_r, domain_r, az, zen)
        assert viz._pts.dtype == np.float64 and viz._pts.shape == (int(H), int(W), int(S), 3)
        if view == 'a':
            close(viz._pts, g['pts64_a'])
        assert np.abs(viz._pts - g['pts_' + view]).max() <= 2.0 ** -24 * np.abs(g['pts_' + view]).max()      # the float32 points the images belong to
        assert viz.coords.shape == (3, int(H), int(W), int(S)) and np.array_equal(viz.coords[1], viz._pts[..., 1])
        assert np.array_equal(viz.x, viz._pts[..., 0]) and np.array_equal(viz.z, viz._pts[..., 2])
        want_d = np.linalg.norm(np.diff(viz._pts, axis=2), axis=-1)
        close(viz.d[..., :-1], want_d)
        assert (viz.d[..., -1] == 0).all()
        assert np.abs(viz.d - g['d_' + view]).max() <= 1e-5                 # ('d' belongs to the float32-rounded points)
        # the restatement's step of row 0 is the reference's d[0] on the rounded points
        p = g['pts_' + view].astype(np.float64)
        close(np.sqrt(((p[0, :, 1:] - p[0, :, :-1]) ** 2).sum(-1)), g['d_' + view][0, :, :-1])


# ---------------------------------------------------------------------------------------------------------------
# 2. argument handling without a device
# ---------------------------------------------------------------------------------------------------------------
def test_render_before_set_view_raises_like_the_reference():
    viz = visualization.VolumeVisualizer(4, 3, 5)
    with pytest.raises(AttributeError, match='must set view before rendering'):
        viz.render(np.zeros((3, 4, 5)), 10.0)


def test_array_cmap_needs_no_matplotlib(monkeypatch):
    for name in [m for m in sys.modules if m == 'matplotlib' or m.startswith('matplotlib.')]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, 'matplotlib', None)                # any import of it now raises ImportError
    monkeypatch.setitem(sys.modules, 'matplotlib.pyplot', None)
    table = np.linspace(0, 1, 12).reshape(4, 3)
    lut = visualization._colour_table(np.concatenate([table, np.ones((4, 1))], axis=1))
    assert lut.dtype == np.float32 and lut.shape == (4, 3) and np.array_equal(lut, table.astype(np.float32))
    with pytest.raises(ImportError):
        visualization._colour_table('no_such_map_' + 'x')
    with pytest.raises(AttributeError):
        visualization._colour_table(np.zeros((1, 3)))
    import torch
    if not torch.cuda.is_available():                                    # the array form reaches the device check: no CPU fallback
        viz = visualization.VolumeVisualizer(4, 3, 5)
        viz.set_view(37.0, 8.0, 0.3, 1.0)
        with pytest.raises(_hip.HipError):
            viz.render(np.zeros((3, 4, 5)), 15.2, cmap=table)
        with pytest.raises(AttributeError):
            viz.render(np.zeros((3, 4, 6)), 15.2, cmap=table)


def test_named_cmap_is_matplotlibs_table():
    pytest.importorskip('matplotlib')
    close(visualization._colour_table('hot'), vc.golden()['lut_hot'].astype(np.float32))


def test_module_is_exported_with_the_references_signatures():
    import inspect
    import bhnerf_amd
    assert bhnerf_amd.visualization is visualization
    V = visualization.VolumeVisualizer
    assert list(inspect.signature(V.__init__).parameters) == ['self', 'width', 'height', 'samples']
    assert list(inspect.signature(V.set_view).parameters) == ['self', 'cam_r', 'domain_r', 'azimuth', 'zenith', 'up']
    assert list(inspect.signature(V.render).parameters) == ['self', 'emission', 'facewidth', 'jit', 'bh_radius', 'linewidth', 'bh_albedo', 'cmap']
    r = inspect.signature(V.render).parameters
    assert (r['jit'].default, r['bh_radius'].default, r['linewidth'].default, r['bh_albedo'].default, r['cmap'].default) == (False, 0.0, 0.1, [0, 0, 0], 'hot')
    for name in ('viewmatrix', 'generate_rays', 'sample_along_rays', 'coords'):
        assert hasattr(V, name)


# ---------------------------------------------------------------------------------------------------------------
# 3. the table
# ---------------------------------------------------------------------------------------------------------------
def test_table_is_well_formed():
    ids = [c.id for c in vc.CASES]
    assert len(set(ids)) == len(ids)
    for c in vc.CASES:
        assert len(c.why) > 10 and c.mutants and all(m in vc.MUTANTS for m in c.mutants), c
    assert {m for c in vc.CASES for m in c.mutants} == set(vc.MUTANTS)
    assert {c.p['S'] for c in vc.CASES} >= {1, 2, 63, 64, 65, 130} and {c.p['lut_n'] for c in vc.CASES} == {2, 256}


@pytest.mark.parametrize('case_id,mutant', [(c.id, m) for c in vc.CASES for m in c.mutants])
def test_case_flags_its_mutant_by_5x_the_bound(case_id, mutant):
    case, inp, wire, ref = prepared(case_id)
    assert vc.error(ref, ref) == 0.0 and np.isfinite(ref).all()
    err = vc.error(vc.reference(case, inp, mutant, wire=wire), ref)
    assert err >= vc.MUTANT_FACTOR * vc.BOUND, vc.report(case, err)


@pytest.mark.parametrize('case_id', ['volume-golden_b', 'volume-S130', 'volume-stub_vertex', 'volume-e_edges'])
def test_bound_is_not_under_the_float32_floor_of_the_restatement(case_id):
    """The same restatement in float32 arithmetic on the same float32 inputs: what single precision costs the reference itself.
    A bound under it would ask the kernel for more than the reference's own arithmetic gives."""
    case, inp, wire, ref = prepared(case_id)
    floor = vc.error(vc.reference(case, inp, dtype=np.float32), ref)
    print('%s: float32 floor %.2e' % (case.id, floor))
    assert floor <= vc.BOUND
    assert vc.BOUND <= 1e-5                 # ... and not so loose that the floor's order of magnitude is lost


def test_input_properties_the_cases_rely_on():
    by = {c.name: c for c in vc.CASES}
    # rays that miss: every sample is zeroed, the reference image is exactly 1
    case, inp, wire, ref = prepared('volume-miss')
    assert (np.abs(inp['pts']).max(-1) > inp['fw'] / 2 + inp['lw']).all() and (ref == 1.0).all()
    # the stub case: the vertex sample is outside the cube, not zeroed, and only the stubs take its alpha to 1
    case, inp, wire, ref = prepared('volume-stub_vertex')
    q = inp['pts'][0, 0, 1].astype(np.float64)
    h = inp['fw'] / 2
    assert (q > h).all() and (q < h + inp['lw']).all() and np.linalg.norm(q - h) < 2 * inp['lw']
    assert wire[0, 0, 1] > 1.0 and vc.wire_alpha(inp['pts'], inp['fw'], inp['lw'], stubs=False)[0, 0, 1] < 0.5
    # the shell case: samples strictly between the two thresholds, some of them on a wire
    case, inp, wire, ref = prepared('volume-shell')
    amax = np.abs(inp['pts'].astype(np.float64)).max(-1)
    shell = (amax > inp['fw'] / 2 - inp['lw']) & (amax < inp['fw'] / 2 + inp['lw'])
    assert shell.sum() >= 8 and (wire[shell] >= 1).any() and (wire[shell] < 1e-3).any()
    # emission edge values, inside the cube
    case, inp, wire, ref = prepared('volume-e_edges')
    e = inp['emission']
    assert (e == 0).any() and (e == 1).any() and ((e > 1) & (e < 1.00001)).any() and (e < 0).any()
    # the black hole is seen from a side where l . p takes both signs
    case, inp, wire, ref = prepared('volume-bh_both_signs')
    p = inp['pts'].astype(np.float64)
    hole = np.linalg.norm(p, axis=-1) < inp['bh']
    lp = (p * np.array([-1.0, -1.0, 1.0])).sum(-1)
    first = hole & (np.cumsum(hole, axis=-1) == 1)                      # the sample that decides the pixel
    assert (lp[first] > 0.2).any() and (lp[first] < -0.2).any()
    # no point sits within float32 rounding of a threshold (there the float64 reference and any float kernel may differ)
    for c in vc.CASES:
        inp = prepared(c.id)[1]
        p = inp['pts'].astype(np.float64)
        amax, norm = np.abs(p).max(-1), np.linalg.norm(p, axis=-1)
        for v, b in ((amax, inp['fw'] / 2 + inp['lw']), (amax, inp['fw'] / 2 - inp['lw'])) + (((norm, inp['bh']),) if inp['bh'] > 0 else ()):
            assert np.abs(v - b).min() > 1e-6 * max(b, 1.0), c
    assert by['N3_padded'].p['pad'] % 4 != 0 and by['misaligned'].p['shift'] == 1


@pytest.mark.parametrize('case_id', [c.id for c in vc.CASES])
def test_case_inputs_are_deterministic_and_float32(case_id):
    case = next(c for c in vc.CASES if c.id == case_id)
    a, b = vc.inputs(case), vc.inputs(case)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == np.float32, k
    assert a['emission'].shape == (a['N'], a['H'], a['W'], a['S']) and a['pts'].shape == (a['H'], a['W'], a['S'], 3)


# ---------------------------------------------------------------------------------------------------------------
# 4. the entry point is declared, exported and bound
# ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_in_the_header_the_export_map_and_the_binding():
    import ctypes as C
    import fnmatch
    import re
    hdr = open(os.path.join(ROOT, 'include', 'bhnerf_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bbhn_volume_render\s*\(', code) and 'bhn_volume_view' in code and '33 entry points' in hdr
    emap = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'bhnerf_amd', 'csrc', 'export.map')).read(), flags=re.S)
    patterns = re.search(r'global:\s*([^;]+);', emap).group(1).split()
    assert any(fnmatch.fnmatchcase('bhn_volume_render', pat) for pat in patterns)
    assert 'volume_render.hip' in open(os.path.join(ROOT, 'bhnerf_amd', 'csrc', 'Makefile')).read()
    res, args = _hip.SIGNATURES['bhn_volume_render']
    assert res is C.c_int and len(args) == 13 and args[10] is C.POINTER(_hip.bhn_volume_view)
    assert C.sizeof(_hip.bhn_volume_view) == 48 and [f[0] for f in _hip.bhn_volume_view._fields_] == ['facewidth', 'linewidth', 'bh_radius', 'bh_albedo']
    assert len(_hip.SIGNATURES) == 33
