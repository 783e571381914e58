"""GPU tests of every render path at four Stokes planes (I, Q, U, V: what kgeo.py and bhn_grf_transport produce whenever V_frac != 0).
The cases, why each is there (the branch, and the LDS bytes of its kernels at Sx = 4), the comparator and the bounds live in
tests/stokes4_cases.py, the references in tests/mlp_reference.py (Reference: the emission on the in-domain points); tests/test_stokes4_cases_cpu.py proves on the CPU that these bounds see a lost, aliased or
mis-strided fourth plane.  Each case, per arithmetic mode:

* runs twice on fresh predictors and is bitwise equal to itself;
* f32: per-plane image figure (error of plane s over the largest entry of the float64 oracle's |J| image of that plane) below
  IMG_TOL['f32'], gradient below GTOL / L2TOL['f32'] against the float64 oracle, ReLU ties adjudicated by
  mlp_bounds.held_or_adjudicated;
* bf16: per-plane image figure against the float64 oracle below IMG_TOL['bf16']; whole-image error, gradient and worst tensor against
  the emulator of the recipe that ran (gpu_support.assert_path) inside 4x the
  figures observed on the MI355X (mlp_bounds.OBSERVED under the case's name), never above the caps of its class; 8x256 (class 'deep',
  no cap): the float64 gradient bounds and 4x the figures of the same network at three planes;
* planes 0 to 2 of the S = 4 render equal the S = 3 render of the same problem without the V row: bit for bit on a dense layout (a
  plane's sums do not depend on the other planes), to f32 rounding on a point-compacted one.

'chi2' cases go through the reference-shaped API (gpu_support.chi2_step: network.loss_fn_image and its backward, chi2_image on
B * Sx blocks); 'linear' cases through eng.render / render_train and eng.render_bwd / render_bwd_tape with an upstream gradient that
differs in every frame and plane, both routes held to the references (and, where the case says so, to each other bit for bit).
"""
import numpy as np
import pytest
import torch

import stokes4_cases as sc
from gpu_support import assert_path, chi2_step, dev, device_setup, ray_args  # noqa: F401
from mlp_bounds import held_or_adjudicated

pytestmark = pytest.mark.gpu

PARAMS = [(name, mode) for name, c in sc.CASES.items() for mode in c['modes']]


def assert_case_path(name, mode, eng, geom):
    """gpu_support.assert_path of a case, and the ray sums it is listed for."""
    c = sc.CASES[name]
    assert_path(name, eng, geom, mode, sc.case_recipe(name, mode), c['general'], compact=c['compact'], tile_groups=c.get('tile_groups'))
    assert geom.S == 4 and geom.Sx == 4, (name, 'layout')
    # direct adds or the combine through LDS (fused_fwd.hip fused_fill_args: ray_direct)
    direct = geom.compact['ray_span'] in (1, 2) if c['compact'] else geom.G <= 33 or (geom.G <= 64 and geom.G % 32 == 0)
    assert direct == c['direct'], (name, 'ray_direct', direct)


def device_outputs(dev, name, mode, prob):
    """One run of a case on a fresh predictor -> a list of outputs in stokes4_cases.outputs' layout, one per route ('chi2': the
    chi^2 step; 'linear': render_train + render_bwd_tape, render + render_bwd), and the plain render (B, 4, R) as a tensor."""
    c, g = sc.CASES[name], prob['g']
    pred, eng, geom, flat, tM0 = device_setup(g, mode, dev)
    assert_case_path(name, mode, eng, geom)
    B = len(g['t_frames'])
    eng.pack(flat)
    rendered = eng.render(geom, tM0).clone()
    assert tuple(rendered.shape) == (B, 4, geom.R)
    npy = lambda t: t.detach().cpu().numpy().astype(np.float64)
    if c['kind'] == 'chi2':
        _, images, grad = chi2_step(pred, flat, ray_args(g), g['t_frames'], prob['target'], prob['sigma'], prob['offset'], 1.0, c['dt'])
        assert tuple(images.shape) == (B, 4) + tuple(prob['spatial'])
        return [dict(images=npy(images).reshape(B, 4, -1), grad=grad.astype(np.float64))], rendered
    train = eng.render_train(geom, tM0).clone()
    dimg = prob['dimg'].float().to(dev).contiguous()
    assert tuple(dimg.shape) == (B, 4, geom.R)
    g_tape = eng.render_bwd_tape(geom, tM0, dimg).clone()
    g_rec = eng.render_bwd(geom, tM0, dimg).clone()
    if c['routes_bitwise']:
        assert torch.equal(rendered, train), (name, 'render != render_train')
        assert torch.equal(g_tape, g_rec), (name, 'recorded tape != recompute')
    return [dict(images=npy(train), grad=npy(g_tape)), dict(images=npy(rendered), grad=npy(g_rec))], rendered


def three_plane_render(dev, mode, prob):
    pred, eng, geom, flat, tM0 = device_setup(sc.three_planes(prob['g']), mode, dev)
    assert geom.S == 3
    eng.pack(flat)
    return eng.render(geom, tM0).clone()


def evaluate(dev, name, mode, drop=None):
    """A case in a mode (drop: without these ray samples) -> (the worst figures over its routes, whether two runs agreed bit for bit,
    whether planes 0 to 2 equal the three-plane render: 'bitwise', 'rounding' (compacted layouts, <= 2e-6 of the largest entry) or no,
    its references, the line it printed)."""
    r = sc.case_references(name, mode, drop)
    prob = r['prob']
    outs, rendered = device_outputs(dev, name, mode, prob)
    again, rendered2 = device_outputs(dev, name, mode, prob)
    repro = torch.equal(rendered, rendered2) and all(np.array_equal(a[k], b[k]) for a, b in zip(outs, again) for k in ('images', 'grad'))
    figs = [sc.figures(o, r['ref64'], r['ref_abs'], r['cuts'], r['emu']) for o in outs]
    worst = {k: (np.max([f[k] for f in figs], axis=0).tolist() if k == 'planes' else max(f[k] for f in figs)) for k in figs[0]}
    three = three_plane_render(dev, mode, prob)
    if torch.equal(rendered[:, :3], three):
        planes012 = 'bitwise'
    else:
        close = float((rendered[:, :3] - three).abs().max()) <= 2e-6 * float(three.abs().max())
        planes012 = 'rounding' if close and sc.CASES[name]['compact'] else 'NO'
    line = '\n[stokes4] %-24s %-5s %-9s %s  repeat bitwise %s  planes 0-2 vs S = 3: %s%s' % (
        name, mode, sc.case_recipe(name, mode) or 'f32', sc.describe(worst), repro, planes012, '' if drop is None else '  [tied samples taken out]')
    print(line)
    return worst, repro, planes012, r, line


@pytest.mark.parametrize('name,mode', PARAMS)
def test_four_stokes_planes(dev, name, mode):
    b = sc.bounds(name, mode)
    fig, repro, planes012, r, line = evaluate(dev, name, mode)
    ok, _ = held_or_adjudicated('%s, %s' % (name, mode), (fig, repro, planes012), lambda run: sc.within(run[0], b),
                                lambda: (r['r64'] if mode == 'f32' else r['rem']).relu_ties(r['prob']['g']),
                                lambda ties: evaluate(dev, name, mode, drop=ties)[:3], lambda run: run[1] and run[2] != 'NO')
    assert ok, (line, {k: v for k, v in sc.ratios(fig, b).items() if v >= 1.0}, b)
    assert repro, (name, mode, 'two runs differ')
    assert planes012 != 'NO', (name, mode, 'planes 0 to 2 differ from the three-plane render')
