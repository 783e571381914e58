#!/opt/conda/bin/python3.9
"""Golden vectors of VolumeVisualizer (fixture g13_volume.npz), from the REFERENCE's own visualization.py.

Run in the build container only (the reference never travels to the GPU box):

    /opt/conda/bin/python3.9 tests/golden/make_volume.py

How: as tests/golden/make_golden.py loads the other modules -- visualization.py is loaded unmodified through importlib with
``jax.numpy`` = NumPy (float64), ``jax.jit`` the identity and the named-dimension stand-in for xarray (plus a no-op
``register_dataarray_accessor``); matplotlib is the real one (the 'hot' table is matplotlib's own).  Its ``set_view``,
``render(jit=False)`` (draw_cube, draw_bh) and ``alpha_composite`` then run in float64.

After ``set_view`` the points are rounded to float32 and ``d`` is recomputed by the reference's own expression, and the
emission is float32 as well: the recorded images belong to float32-representable inputs, which is what the device gets.
View a also keeps the unrounded points (``pts64``) so that the package's own ``set_view`` can be held to 1e-12.
Only data is committed.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings('ignore')
REF = '/root/reference/bhnerf'
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import xr_standin  # noqa: E402

import matplotlib  # noqa: E402
matplotlib.use('Agg')


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


jax = _mod('jax', numpy=np, jit=lambda f=None, **kw: (f if f is not None else (lambda g: g)))
sys.modules['jax.numpy'] = np
xr = _mod('xarray', DataArray=xr_standin.DataArray, Dataset=xr_standin.Dataset, register_dataarray_accessor=lambda name: (lambda cls: cls))
pkg = types.ModuleType('bhnerf')
pkg.__path__ = [REF]
sys.modules['bhnerf'] = pkg


def _load(name):
    spec = importlib.util.spec_from_file_location('bhnerf.' + name, os.path.join(REF, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['bhnerf.' + name] = mod
    setattr(pkg, name, mod)
    spec.loader.exec_module(mod)
    return mod


utils = _load('utils')
vis = _load('visualization')

DOMAIN_R, CAM_R, LINEWIDTH = 8.0, 37.0, 0.1
FACEWIDTH = 1.9 * DOMAIN_R
BH_RADIUS, BH_ALBEDO = 2.0, [0.9, 0.6, 0.3]
VIEWS = {'a': dict(W=12, H=10, S=70, azimuth=0.6, zenith=1.1), 'b': dict(W=24, H=16, S=33, azimuth=-2.2, zenith=0.7)}


def emission_at(pts):
    """A hotspot, a fainter arc and a weak floor: values in [0, 1), the maximum inside the cube, non-zero outside it too (so
    that the zeroing of draw_cube acts on something)."""
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    hot = np.exp(-((x - 4.0) ** 2 + (y + 1.0) ** 2 + (z - 0.5) ** 2) / (2 * 1.3 ** 2))
    r = np.sqrt(x ** 2 + y ** 2)
    arc = 0.45 * np.exp(-((r - 5.5) ** 2 + z ** 2) / (2 * 0.9 ** 2)) * (0.5 + 0.5 * np.cos(np.arctan2(y, x) - 2.0))
    return 0.97 * hot + arc * (1 - hot) + 0.02 * np.exp(-np.sqrt(x ** 2 + y ** 2 + z ** 2) / 20.0)


def main():
    import matplotlib.pyplot as plt
    out = dict(lut_hot=plt.get_cmap('hot')(np.arange(256))[:, :3],
               params=np.array([DOMAIN_R, CAM_R, FACEWIDTH, LINEWIDTH, BH_RADIUS] + BH_ALBEDO))
    for name, v in VIEWS.items():
        viz = vis.VolumeVisualizer(v['W'], v['H'], v['S'])
        viz.set_view(CAM_R, DOMAIN_R, v['azimuth'], v['zenith'])
        pts64 = np.asarray(viz._pts, dtype=np.float64)
        assert pts64.shape == (v['H'], v['W'], v['S'], 3)
        pts = pts64.astype(np.float32)
        viz._pts = pts.astype(np.float64)
        viz.x, viz.y, viz.z = viz._pts[..., 0], viz._pts[..., 1], viz._pts[..., 2]
        viz.d = np.linalg.norm(np.concatenate([np.diff(viz._pts, axis=2), np.zeros_like(viz._pts[..., -1:, :])], axis=2), axis=-1)   # visualization.py:541-543
        e = emission_at(viz._pts).astype(np.float32)
        assert 0.0 < e.min() and 0.5 < e.max() < 1.0
        out.update({'view_' + name: np.array([v['W'], v['H'], v['S'], v['azimuth'], v['zenith']]), 'pts_' + name: pts, 'd_' + name: viz.d,
                    'emission_' + name: e})
        if name == 'a':
            out['pts64_a'] = pts64
        e64 = e.astype(np.float64)
        out['image_%s_nobh' % name] = np.asarray(viz.render(e64, FACEWIDTH, jit=False, bh_radius=0.0, linewidth=LINEWIDTH, cmap='hot'))
        out['image_%s_bh' % name] = np.asarray(viz.render(e64, FACEWIDTH, jit=False, bh_radius=BH_RADIUS, linewidth=LINEWIDTH, bh_albedo=BH_ALBEDO, cmap='hot'))
        for k in ('nobh', 'bh'):
            img = out['image_%s_%s' % (name, k)]
            assert img.dtype == np.float64 and img.shape == (v['H'], v['W'], 3) and np.isfinite(img).all()
            print(name, k, 'image range %.4g .. %.4g' % (img.min(), img.max()))
    path = os.path.join(OUT, 'g13_volume.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
