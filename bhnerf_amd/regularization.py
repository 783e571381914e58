"""Priors on the recovered 3-D emission: smoothed isotropic total variation ('tv'), total squared variation ('tsv') and the l1
norm ('l1') of the emission sampled on a fixed regular lattice (libbhnerf_reg.so, include/bhnerf_reg.h).

The reference carried ``network.tv_reg(apply_fn, params, coords)``, the mean absolute gradient of the emission by autodiff at the
given points; it never ran (``lam`` is undefined at network.py:931).  ``VolumePrior`` is that intent with finite differences: the
network is sampled on the lattice as ``network.sample_3d_grid`` samples it (no warp, nothing before injection), the prior is one
loss kernel with a gradient in the sampled volume, and the fused backward carries that gradient to the parameters
(``network.gradient_step_volume``, ``optimization.TrainStep.volume_prior``).
"""
import numpy as np

from .observation import term_weights

REG_TERMS = ('tv', 'tsv', 'l1')                     # the canonical order of the terms


def _regular_axis(values, name):
    """Spacing of a strictly increasing, evenly spaced 1-D axis (1.0 for a single point); AttributeError otherwise."""
    values = np.asarray(values, dtype=np.float64)
    if values.size == 1:
        return 1.0
    steps = np.diff(values)
    h = float(values[-1] - values[0]) / (values.size - 1)
    # (coordinates that were rounded to float32 are even to ~1e-7 of their size, not of their spacing)
    if not (np.isfinite(h) and h > 0) or np.abs(steps - h).max() > 1e-6 * (h + np.abs(values).max()):
        raise AttributeError('coords are not a regular lattice: the {} axis is not evenly spaced and increasing'.format(name))
    return h


class VolumePrior:
    """The lattice, weights and smoothing of a volume prior -- the operator ``engine.chi2_volume`` takes.

    The lattice is ``fov`` in M with ``resolution`` (an int or a triple; ``np.linspace(-fov / 2, fov / 2, resolution)`` per axis,
    as in ``network.sample_3d_grid``), or a regular ``coords`` (3, nx, ny, nz) in ``np.meshgrid(.., indexing='ij')`` order; an
    irregular one raises AttributeError.  ``weights``: {'tv' | 'tsv' | 'l1': w >= 0}, a missing term is absent; unknown keys raise
    AttributeError.  ``eps``: the smoothing of tv, sqrt(|grad e|^2 + eps^2), in emission per M.  ``normalize``: each weight is
    divided by the number of in-domain voxels of the call, so that a weight means the same at every resolution (the reference's
    tv_reg is a mean too); a call with no in-domain voxel raises AttributeError.

    After a call ``last_terms`` holds the four floats {total, tv, tsv, l1} (a device tensor: reading it synchronises) and, after
    a step of ``network.gradient_step_volume`` / ``test_volume``, ``last_volume`` the sampled (nx, ny, nz) emission."""

    def __init__(self, fov=None, resolution=64, coords=None, weights=None, eps=1e-6, normalize=True):
        if coords is None and fov is None:
            raise AttributeError('Either coords or fov+resolution must be provided')
        if coords is None:
            res = np.atleast_1d(np.asarray(resolution))
            if res.size not in (1, 3) or res.dtype.kind not in 'iu' or np.any(res < 1):
                raise AttributeError('resolution ({}) should be a positive int or three of them'.format(resolution))
            half = np.atleast_1d(np.asarray(fov, dtype=np.float64)) / 2
            if half.size not in (1, 3) or not np.all(np.isfinite(half)) or np.any(half <= 0):
                raise AttributeError('fov ({}) should be positive and finite'.format(fov))
            axes = [np.linspace(-h, h, int(n)) for h, n in zip(np.broadcast_to(half, 3), np.broadcast_to(res, 3))]
            coords = np.array(np.meshgrid(*axes, indexing='ij'))
        else:
            coords = np.asarray(coords, dtype=np.float64)
            if coords.ndim != 4 or coords.shape[0] != 3 or coords.size == 0:
                raise AttributeError('coords {} should be (3, nx, ny, nz)'.format(coords.shape))
            axes = [coords[0][:, 0, 0], coords[1][0, :, 0], coords[2][0, 0, :]]
            if not np.array_equal(np.array(np.meshgrid(*axes, indexing='ij')), coords):
                raise AttributeError("coords are not a regular lattice in np.meshgrid(.., indexing='ij') order")
        self.dims = tuple(int(n) for n in coords.shape[1:])
        self.spacing = tuple(_regular_axis(a, n) for a, n in zip(axes, 'xyz'))
        # (3, nx, ny, nz, 1): one sample per "ray".  ONE array for the life of the operator: the geometry cache keys on its identity
        self.coords = np.ascontiguousarray(coords[..., None], dtype=np.float32)
        self.weights = tuple(term_weights(REG_TERMS, {'tv': 1.0} if weights is None else weights, 0.0).values())
        self.eps = float(eps)
        if self.weights[0] != 0 and not (np.isfinite(self.eps) and self.eps > 0):
            raise AttributeError('eps ({}) must be positive and finite when the tv weight is not 0'.format(eps))
        self.normalize = bool(normalize)
        self.last_terms = self.last_per_volume = self.last_volume = None
        self._count = None                              # (mask, its version, in-domain voxels) of the last call

    @property
    def num_voxels(self):
        return int(np.prod(self.dims))

    def in_domain(self, mask):
        """Number of voxels in `mask` (None: all); a device mask is counted once per mask object and version."""
        if mask is None:
            return self.num_voxels
        hit = self._count
        version = getattr(mask, '_version', None)
        if hit is not None and hit[0] is mask and hit[1] == version and version is not None:
            return hit[2]
        count = int(mask.sum().item()) if hasattr(mask, 'is_cuda') else int(np.count_nonzero(mask))
        self._count = (mask, version, count)
        return count

    def call_weights(self, mask):
        """The weights of a call on `mask`, in the canonical order; AttributeError when normalising by zero voxels."""
        if not self.normalize:
            return self.weights
        count = self.in_domain(mask)
        if count == 0:
            raise AttributeError('the prior is normalised by the number of in-domain voxels and the mask has none')
        return tuple(w / count for w in self.weights)
