"""Volume rendering of the recovered 3-D emission (the reference's ``bhnerf.visualization.VolumeVisualizer``).

``set_view`` is the reference's host NumPy (visualization.py:510-543, 593-626); ``render`` (visualization.py:545-591 with
draw_cube, draw_bh and alpha_composite) is one HIP kernel, ``bhn_volume_render`` (csrc/volume_render.hip): there is no
CPU fallback.  Differences from the reference, also listed in INTEGRATION.md:

  * an all-zero frame renders with alpha 0 for the emission (the reference divides by ``amax = 0`` and returns NaN);
  * a 4-D ``emission`` (N, H, W, S) renders N frames in one launch, each normalised by its own maximum;
  * the image is float32.
"""
import numpy as np
import torch

from . import _hip

_LUTS = {}
normalize = lambda vector: vector / np.sqrt(np.dot(vector, vector))       # utils.py:13


def _colour_table(cmap):
    """(n, 3) float32 colour table: a matplotlib name (imported only then) or an (n, 3|4) array used as it is."""
    if isinstance(cmap, str):
        if cmap not in _LUTS:
            import matplotlib.pyplot as plt
            cm = plt.get_cmap(cmap)
            _LUTS[cmap] = np.ascontiguousarray(cm(np.arange(cm.N))[:, :3], dtype=np.float32)
        return _LUTS[cmap]
    if hasattr(cmap, 'N') and callable(cmap):              # a matplotlib Colormap object
        return np.ascontiguousarray(cmap(np.arange(cmap.N))[:, :3], dtype=np.float32)
    lut = np.asarray(cmap, dtype=np.float32)
    if lut.ndim != 2 or lut.shape[1] not in (3, 4) or lut.shape[0] < 2:
        raise AttributeError('cmap must be a matplotlib name or an (n >= 2, 3|4) array, got shape {}'.format(lut.shape))
    return np.ascontiguousarray(lut[:, :3])


class VolumeVisualizer(object):
    def __init__(self, width, height, samples):
        """width, height: camera resolution; samples: integration points along a ray."""
        self.width = width
        self.height = height
        self.samples = samples
        self._pts = None
        self._pts_dev = {}

    def set_view(self, cam_r, domain_r, azimuth, zenith, up=np.array([0., 0., 1.])):
        """Camera at distance cam_r looking at the origin; domain_r: radius of the spherical domain (angles in radians)."""
        camorigin = cam_r * np.array([np.cos(azimuth) * np.sin(zenith),
                                      np.sin(azimuth) * np.sin(zenith),
                                      np.cos(zenith)])
        self._viewmatrix = self.viewmatrix(camorigin, np.asarray(up, dtype=np.float64), camorigin)
        fov = 1.06 * np.arctan(np.sqrt(3) * domain_r / cam_r)
        focal = .5 * self.width / np.tan(fov)
        rays_o, rays_d = self.generate_rays(self._viewmatrix, self.width, self.height, focal)
        near = cam_r - np.sqrt(3) * domain_r
        far = cam_r + np.sqrt(3) * domain_r
        self._pts = self.sample_along_rays(rays_o, rays_d, near, far, self.samples)
        self.x, self.y, self.z = self._pts[..., 0], self._pts[..., 1], self._pts[..., 2]
        self.d = np.linalg.norm(np.concatenate([np.diff(self._pts, axis=2), np.zeros_like(self._pts[..., -1:, :])], axis=2), axis=-1)
        self._pts_dev = {}

    def viewmatrix(self, lookdir, up, position):
        """Construct lookat view matrix."""
        vec2 = normalize(lookdir)
        vec0 = normalize(np.cross(up, vec2))
        vec1 = normalize(np.cross(vec2, vec0))
        return np.stack([vec0, vec1, vec2, position], axis=1)

    def generate_rays(self, camtoworlds, width, height, focal):
        """Pixel-centre rays.  The camera-frame directions are float32, as in the reference (float32 pixel grids divided by
        the focal length: float32 under JAX and under NumPy's scalar rules alike); the rotation to the world is float64."""
        x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32), indexing='xy')
        f32 = np.float32
        camera_dirs = np.stack([(x - f32(width * 0.5) + f32(0.5)) / f32(focal),
                                -(y - f32(height * 0.5) + f32(0.5)) / f32(focal), -np.ones_like(x)], axis=-1)
        directions = (camera_dirs[..., None, :] * camtoworlds[None, None, :3, :3]).sum(axis=-1)
        origins = np.broadcast_to(camtoworlds[None, None, :3, -1], directions.shape)
        return origins, directions

    def sample_along_rays(self, rays_o, rays_d, near, far, num_samples):
        t_vals = np.linspace(near, far, num_samples)
        return rays_o[..., None, :] + t_vals[None, None, :, None] * rays_d[..., None, :]

    @property
    def coords(self):
        """(3, H, W, S) sample points, for network.sample_3d_grid(coords=...) and emission.interpolate_coords."""
        return None if self._pts is None else np.moveaxis(self._pts, -1, 0)

    def _device_points(self, dev):
        key = (dev.type, dev.index)
        if key not in self._pts_dev:
            self._pts_dev[key] = _hip.as_f32(self._pts, dev)
        return self._pts_dev[key]

    def render(self, emission, facewidth, jit=False, bh_radius=0.0, linewidth=0.1, bh_albedo=[0, 0, 0], cmap='hot'):
        """RGB image (H, W, 3) of the emission sampled at ``coords`` -- (H, W, S), or (N, H, W, S) for N images from one
        launch -- inside a wireframe cube of face ``facewidth``, with a sphere of ``bh_radius`` shaded by ``bh_albedo``.
        ``jit`` is accepted for the reference's signature and ignored.  NumPy in, NumPy out; torch in, torch out."""
        if self._pts is None:
            raise AttributeError('must set view before rendering')
        lut = _colour_table(cmap)
        H, W, S = self._pts.shape[:3]
        is_torch = isinstance(emission, torch.Tensor)
        shape = tuple(emission.shape)
        if shape[-3:] != (H, W, S) or len(shape) not in (3, 4):
            raise AttributeError('emission shape {} does not match the view ({}, {}, {})'.format(shape, H, W, S))
        if is_torch and emission.is_cuda:
            dev = emission.device
        elif torch.cuda.is_available():
            dev = torch.device('cuda', torch.cuda.current_device())
        else:
            raise _hip.HipError('VolumeVisualizer.render runs on the HIP device only (no CPU fallback)')
        em = _hip.as_f32(emission, dev).reshape((-1, H, W, S))
        N = em.shape[0]
        amax = em.reshape(N, -1).amax(dim=1)
        alpha_scale = torch.where(amax != 0, 1.0 / amax, torch.zeros_like(amax)).contiguous()      # on the device: no host sync
        images = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev)
        view = _hip.bhn_volume_view(float(facewidth), float(linewidth), float(bh_radius), (_hip.C.c_double * 3)(*[float(a) for a in bh_albedo]))
        lut_dev = torch.as_tensor(lut, device=dev)
        _hip.check(_hip.lib().bhn_volume_render(_hip.ptr(self._device_points(dev)), _hip.ptr(em), _hip.ptr(alpha_scale), N, H, W, S, H * W * S,
                                                _hip.ptr(lut_dev), lut.shape[0], _hip.C.byref(view), _hip.ptr(images), _hip.stream_ptr(dev)))
        out = images if len(shape) == 4 else images[0]
        return out if is_torch else out.cpu().numpy()
