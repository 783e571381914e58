"""The case table of the stand-alone kernels (bhnerf_amd/csrc/simple_kernels.hip), shared by
tests/test_gpu_standalone_kernels.py (runs each case on the device) and tests/test_standalone_refs_cpu.py (proves on the
CPU that each case's comparator and bound see the slips the case is for).  NumPy only.

A case is (family, id, parameters, `why`: the branch of the kernel it is for, mutants).  For every case
    inputs(case)              -> dict of float32 (or float64 / uint8 where the ABI says so) arrays, deterministic
    reference(case, inp)      -> dict name -> float64 output, from the float32-rounded inputs
    reference(case, inp, m)   -> the same with slip `m` built in (MUTANTS)
    scales(case, inp, ref)    -> dict name -> denominator, a quantity of the reference alone
    errors(case, got, ref, sc)-> dict name -> (observed, bound)
Bounds are the ones the existing tests hold each kernel to (BOUNDS).  Outputs compared for equality ('dom') have
bound 0 and `observed` = the number of differing entries.

Denominators are the largest entry of the reference, as the existing tests measure each kernel (the EHT loss and gradient
included: the visibility sums of both signs meet the result-relative 2e-5 as they stand).  The one exception is the
Stokes-weighted grid gradient, a scatter-sum of signed terms: there the denominator is the reference evaluated on
|dimages| and |w| (a float32 sum of n terms is off by ~n 2^-24 sum|terms| whatever the result).
"""
import zlib

import numpy as np

from oracle import oracle_np as onp

SENTINEL = -777.25            # pre-fill of every output buffer and its guard bands
GUARD = 64                    # elements of guard band before and after every output

BOUNDS = {                    # kernel family -> output -> bound, each from the test that already holds it
    'geom': {'w': 1e-6, 'dom': 0.0},                                   # test_gpu_forward.test_geom_prepare
    'rt': {'img': 2e-6, 'de': 2e-6},                                   # test_gpu_forward.test_radiative_transfer_standalone
    'chi2_full': {'loss0': 1e-5, 'loss_planes': 1e-5, 'dimg': 1e-5},   # test_gpu_forward.test_chi2_and_adam
    'chi2_lc': {'loss0': 1e-4, 'loss_planes': 1e-4, 'dimg': 1e-4},
    'adam': {'p': 1e-5, 'm': 1e-5, 'v': 1e-5},
    'eht': {'loss0': 2e-5, 'dimg': 2e-5},                              # test_gpu_eht
    'trilinear': {'out': 2e-6},                                        # test_gpu_voxel.test_interpolate_coords_golden
    'voxel': {'images': 2e-5},                                         # test_gpu_voxel (at size)
    'grid': {'emission': 1e-5, 'images': 1e-5, 'dgrid': 1e-4},         # test_gpu_grid
}

# Constants of the kernels the shapes below are chosen from
GEOM_CAP = 4096 * 256         # geom_prepare_kernel: grid-stride past this many points
ADAM_CAP = 1024 * 256         # adam_kernel
TRI_CAP = 2048 * 256          # trilinear_kernel
LOSS_SUM_STRIDE = 256         # loss_sum_kernel: one block of 256 threads strides over the partial terms
EHT_LOSS_BLOCK = 256          # eht_loss_kernel: (frame, visibility) terms per block


class Case:
    def __init__(self, family, name, why, mutants=(), **p):
        self.family, self.name, self.why, self.mutants, self.p = family, name, why, tuple(mutants), p
        self.id = family + '-' + name

    def __repr__(self):
        return self.id

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.id.encode()))

    @property
    def bounds(self):
        fam = self.family
        if fam == 'chi2':
            fam = 'chi2_full' if self.p['dtype'] == 'full' else 'chi2_lc'
        return BOUNDS[fam]


f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
f64 = lambda a: np.asarray(a, dtype=np.float64)
r32 = lambda v: float(np.float32(v))          # a scalar the ABI takes as float


# ===============================================================================================================
# EHT: the R-axis split of the visibility GEMV is a pure function of (rows, R): restated, and asserted per case
# ===============================================================================================================
def eht_splits(rows, R):
    rs = (2048 + rows - 1) // rows
    most = max(R // 2048, 1)
    return int(max(1, min(rs, most, 64)))


def eht_span(R, RS):
    return ((R + RS - 1) // RS + 1) & ~1


# ===============================================================================================================
# the table
# ===============================================================================================================
def _cases():
    C = []
    add = lambda *a, **k: C.append(Case(*a, **k))
    # ---- bhn_geom_prepare ----
    add('geom', 'gridstride_S4', 'P = 4096*256 + 1061 points: second grid-stride trip of geom_prepare_kernel, P % 256 != 0, S = 4',
        ('skip_second_trip',), P=GEOM_CAP + 1061, S=4, exact=False)
    add('geom', 'boundary_equal', 'r^2 == rmin^2, r^2 == rmax^2, |z| == z_width exactly (all inclusive), S = 0, P % 256 != 0',
        ('exclusive_bounds',), P=333, S=0, exact=True)
    add('geom', 'one_point', 'P = 1: one thread of one block live; the point has r^2 == rmin^2', ('exclusive_bounds',), P=1, S=1, exact=True)
    # ---- bhn_radiative_transfer_fwd / _bwd: (N, R, G, shift of every array in floats) ----
    rt = lambda name, why, mut, N, R, G, shift=0, shift_out=None: add('rt', name, why, mut, N=N, R=R, G=G, shift=shift, shift_out=shift if shift_out is None else shift_out)
    rt('lpr1_g3', 'G <= 4: LPR = 1, 256 rays per block, second block + ray tail, scalar path', ('drop_last_sample', 'drop_tail4', 'skip_second_block'), 2, 300, 3)
    rt('lpr1_g4_vec', 'G = 4 aligned: LPR = 1 on the 16-byte path', ('drop_last_sample', 'skip_second_block'), 2, 257, 4)
    rt('lpr2_g5', 'G = 5: LPR = 2, a block holds 128 rays: ray tail and second block', ('drop_last_sample', 'drop_tail4', 'skip_second_block'), 3, 165, 5)
    rt('lpr4_g13', 'G 9..16: LPR = 4, 64 rays per block, scalar tail G % 4 = 1', ('drop_last_sample', 'drop_tail4', 'skip_second_block'), 2, 70, 13)
    rt('lpr8_g32_vec', 'G 17..32: LPR = 8 on the 16-byte path, 32 rays per block', ('drop_last_sample', 'skip_second_block'), 2, 45, 32)
    rt('kch3_g700_vec', 'G 513..768: LPR = 64, KCH = 3 on the 16-byte path', ('drop_last_sample',), 2, 9, 700)
    rt('kch3_g767', 'G 513..768: LPR = 64, KCH = 3, scalar path with a 3-element tail', ('drop_last_sample', 'drop_tail4'), 1, 6, 767)
    rt('g64_misaligned', 'G % 4 == 0 on a 4-byte aligned sub-view: must take the scalar path', ('drop_last_sample',), 2, 21, 64, shift=1)
    rt('g64_out_misaligned', 'G % 4 == 0, inputs 16-byte aligned, only the outputs on a 4-byte aligned sub-view: the output pointer is part of the alignment test', ('drop_last_sample',), 2, 21, 64, shift_out=1)
    rt('g1', 'G = 1: one sample per ray, LPR = 1', ('drop_last_sample', 'skip_second_block'), 2, 259, 1)
    rt('g1024', 'G = 1024: the largest accepted, LPR = 64, KCH = 4', ('drop_last_sample',), 2, 5, 1024)
    # ---- bhn_chi2_image ----
    ci = lambda name, why, mut, dtype, B, S, R, shift=0, grad=True, shift_out=None, **k: add('chi2', name, why, mut, dtype=dtype, B=B, S=S, R=R, shift=shift,
                                                                                             shift_out=shift if shift_out is None else shift_out, grad=grad, **k)
    ci('full_scalar_multitrip', "R = 4099 > 4096, R % 4 = 3: scalar path, five trips of 1024 threads", ('drop_tail4', 'skip_second_trip_r'), 'full', 2, 2, 4099)
    ci('full_vec_multitrip', 'R = 8204, R % 4 == 0, aligned: 16-byte path, three trips of 4096 with a short last one', ('skip_second_trip_r',), 'full', 2, 1, 8204)
    ci('full_misaligned', 'R % 4 == 0 on a 4-byte aligned sub-view: scalar path', ('skip_second_trip_r',), 'full', 1, 3, 4100, shift=1)
    ci('full_out_misaligned', 'R % 4 == 0, inputs 16-byte aligned, only dimages on a 4-byte aligned sub-view: scalar path (dimages is part of the alignment test)', ('skip_second_trip_r',), 'full', 1, 2, 4100, shift_out=1)
    ci('full_R3', 'R < 4: three of 1024 threads live', ('drop_tail4',), 'full', 2, 2, 3)
    ci('full_R1', 'R = 1: one pixel per plane, one live thread', ('drop_tail4',), 'full', 3, 1, 1)
    ci('full_300_planes', 'B*S = 300 planes > 256: loss_sum_kernel strides', ('skip_second_trip_sum',), 'full', 100, 3, 5)
    ci('full_nograd', "dimages = NULL, 'full'", ('drop_tail4',), 'full', 2, 2, 77, grad=False)
    ci('lc_cancel', "'lc' sums of both signs that cancel to 1e-5 of sum|pixels| (why the kernel sums in double), 16-byte path",
       ('f32_sum',), 'lc', 2, 2, 65536, cancel=True)
    ci('lc_cancel_scalar', "'lc' cancelling sums on the scalar path, R % 4 = 1", ('f32_sum', 'drop_tail4'), 'lc', 1, 3, 65537, cancel=True)
    ci('lc_300_planes', "'lc' with 300 planes: loss_sum_kernel strides", ('skip_second_trip_sum',), 'lc', 150, 2, 6)
    ci('lc_nograd', "dimages = NULL, 'lc'", ('drop_tail4',), 'lc', 2, 2, 77, grad=False)
    # ---- bhn_adam_step / _dev / bhn_adam_hyper ----
    ad = lambda name, why, mut, n, t, gs, **k: add('adam', name, why, mut, n=n, t=t, gs=gs, **k)
    ad('gridstride_1p9M', 'n = 1.9 M (an 8x512 network) > 262144: grid-stride loop, n % 256 != 0, small t, grad_scale 0.5',
       ('skip_second_trip', 'bias_t_minus_1', 'ignore_grad_scale'), 1900037, 2, 0.5)
    ad('large_t', 't = 100000: both bias corrections within 1e-30 of 1; warm m, v; grad_scale 4', ('ignore_grad_scale',), 70001, 100000, 4.0, warm=True)
    ad('t1_n255', 't = 1, n = 255: one partial block', ('ignore_grad_scale',), 255, 1, 0.25)
    ad('t3_n1', 'n = 1: one live thread', ('bias_t_minus_1',), 1, 3, 1.0, warm=True)
    # ---- bhn_chi2_eht: shift_img / shift_A in floats ----
    eh = lambda name, why, mut, dtype, N, C_, nvis, R, RS, **k: add('eht', name, why, mut, dtype=dtype, N=N, C=C_, nvis=nvis, R=R, RS=RS, **k)
    eh('vis_odd_rs2', 'rows 1, R = 4097 (odd, just above 2*2048): RS = 2, scalar path, span rounded up to even 2050', ('drop_last_slice', 'drop_last_element', 'dup_boundary'), 'vis', 1, 1, 1, 4097, 2)
    eh('amp_odd_rs64', 'rows 3, R = 131073 (odd): RS = 64, the cap', ('drop_last_slice', 'drop_last_element', 'dup_boundary'), 'amp', 3, 1, 1, 131073, 64)
    eh('cphase_odd_rs3', 'rows 42, R = 6145 (odd): RS = 3, C = 3', ('drop_last_slice', 'drop_last_element', 'dup_boundary', 'closure_short'), 'cphase', 2, 3, 7, 6145, 3)
    eh('vis_below_rs2', 'rows 4, R = 6143 (just below 3*2048): RS = 2', ('drop_last_slice', 'drop_last_element', 'dup_boundary'), 'vis', 2, 1, 2, 6143, 2)
    eh('vis_below_rs1', 'rows 1, R = 4095 (just below 2*2048): RS = 1', ('drop_last_element',), 'vis', 1, 1, 1, 4095, 1)
    eh('vis_even_wide_rs2', 'R = 4098 even, aligned: 16-byte path with RS = 2', ('drop_last_slice', 'dup_boundary'), 'vis', 1, 1, 2, 4098, 2)
    eh('vis_even_img4', 'R = 4098 even but images 4-byte aligned: wide = 0', ('drop_last_slice', 'dup_boundary'), 'vis', 1, 1, 2, 4098, 2, shift_img=1)
    eh('amp_even_A8', 'R = 4098 even but A 8-byte aligned: wide = 0', ('drop_last_slice', 'dup_boundary'), 'amp', 1, 1, 2, 4098, 2, shift_A=2)
    eh('cphase_C1', 'C = 1 closure (1..8 accepted)', ('closure_short',), 'cphase', 2, 1, 3, 300, 1)
    eh('cphase_C8', 'C = 8 closure, the largest accepted', ('drop_last_element', 'closure_short'), 'cphase', 2, 8, 3, 301, 1)
    eh('cphase_C5', 'C = 5: between the tested 1, 3 and 8', ('closure_short',), 'cphase', 1, 5, 4, 64, 1)
    eh('vis_300_terms', 'N*nvis = 300 > 256: two loss_part blocks', ('skip_second_block_terms',), 'vis', 3, 1, 100, 64, 1)
    eh('amp_65600_terms', 'N*nvis = 65600 > 65536: 257 loss_part blocks, loss_sum_kernel strides', ('skip_second_trip_sum',), 'amp', 8, 1, 8200, 8, 1)
    eh('vis_nograd', 'dimages = NULL', ('drop_last_element',), 'vis', 2, 1, 5, 77, 1, grad=False)
    eh('cphase_nograd', 'dimages = NULL, cphase', ('drop_last_element', 'closure_short'), 'cphase', 2, 3, 5, 77, 1, grad=False)
    # ---- bhn_trilinear ----
    add('trilinear', 'noncubic_gridstride', 'nx != ny != nz, three extents, N = 2048*256 + 999 (second grid-stride trip), points on every low/high face',
        ('skip_second_trip', 'swap_strides', 'one_extent', 'upper_face_zero'), n=(5, 9, 17), ext=(8.0, 12.0, 20.0), N=TRI_CAP + 999)
    add('trilinear', 'axis_1_and_2', 'an axis of length 1 and one of length 2', ('swap_strides', 'one_extent', 'upper_face_zero'), n=(1, 2, 6), ext=(4.0, 6.0, 10.0), N=1000)
    add('trilinear', 'misaligned', 'points / output on 4-byte aligned sub-views', ('swap_strides',), n=(4, 3, 5), ext=(2.0, 3.0, 5.0), N=257, shift=1)
    # ---- bhn_voxel_render_fwd ----
    vx = lambda name, why, mut, B, R, G, S, n, ext, per_frame: add('voxel', name, why, mut, B=B, R=R, G=G, S=S, n=n, ext=ext, per_frame=per_frame)
    vx('perframe_lpr4_S4', 'G = 7 < 12: LPR = 4; S = 4; a distinct grid per frame (frame_stride); nx != ny != nz, three extents',
       ('frame0_grid', 'swap_strides', 'one_extent', 'drop_last_sample', 'upper_face_zero'), 3, 100, 7, 4, (6, 10, 14), (10.0, 14.0, 18.0), True)
    vx('single_lpr16_S0', 'G = 20: LPR = 16, S = 0, one grid, ray tail of the last block', ('swap_strides', 'one_extent', 'drop_last_sample'), 2, 37, 20, 0, (7, 5, 3), (12.0, 10.0, 16.0), False)
    vx('perframe_lpr32_S2', 'G = 50: LPR = 32, S = 2, a distinct grid per frame', ('frame0_grid', 'swap_strides', 'drop_last_sample'), 4, 13, 50, 2, (4, 8, 2), (12.0, 16.0, 9.0), True)
    # ---- bhn_grid_predict_fwd / bhn_grid_render_fwd / bhn_grid_render_bwd ----
    gr = lambda name, why, mut, B, R, G, S, res: add('grid', name, why, mut, B=B, R=R, G=G, S=S, res=res)
    gr('lpr4_S3', 'G = 10: LPR = 4; backward with S = 3 (dE = sum_s dI_s w_s); upper-face and outside-the-grid points; dgrid pre-filled with garbage',
       ('stokes0', 'upper_face_zero', 'drop_last_sample'), 2, 70, 10, 3, 5)
    gr('lpr16_res2', 'G = 20: LPR = 16 in all three modes; res = 2; S = 0', ('upper_face_zero', 'drop_last_sample'), 3, 21, 20, 0, 2)
    gr('lpr32_S2', 'G = 50: LPR = 32 in all three modes; S = 2', ('stokes0', 'upper_face_zero', 'drop_last_sample'), 2, 11, 50, 2, 9)
    return C


CASES = _cases()
BY_FAMILY = {}
for _c in CASES:
    BY_FAMILY.setdefault(_c.family, []).append(_c)

# the documented refusals: (entry point, what is wrong, expected code); built by the GPU module from valid arguments
REFUSALS = ['rt_G1025', 'cphase_C0', 'cphase_C9', 'vis_C2', 'grid_res1', 'grid_S5', 'voxel_S5', 'geom_S5', 'voxel_extent0', 'trilinear_extent_neg']


# ===============================================================================================================
# inputs
# ===============================================================================================================
def smooth_grid(rng, n, lo=0.2, hi=1.0):
    """A smooth, anisotropic grid: trilinear sampling in float32 carries an index error of ~2e-7 (n - 1), so the bound of
    2e-6 of the maximum holds only for grids whose slope per cell is a small multiple of range / (n - 1)."""
    ax = [np.linspace(-1.0, 1.0, k) if k > 1 else np.zeros(1) for k in n]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    a = rng.uniform(0.3, 0.7, 6)
    v = 0.5 + 0.2 * np.sin(1.3 * X + a[0]) + 0.15 * np.cos(0.9 * Y + 2 * a[1]) + 0.1 * Z + 0.08 * X * Y - 0.05 * Y * Z + a[2] * 0.1 * Z * Z
    v = (v - v.min()) / max(v.max() - v.min(), 1e-9)
    return lo + (hi - lo) * v


def _points_in_box(rng, N, ext):
    """Points for the samplers: 80 % strictly inside (|c| <= 0.49 extent), 15 % clearly outside on one axis, and every
    low / high face, edge and corner exactly (+-extent/2 is exact in float32: the extents are small integers)."""
    h = 0.5 * np.asarray(ext, dtype=np.float64)
    pts = rng.uniform(-0.98, 0.98, (N, 3)) * h
    out = rng.random(N) < 0.15
    ax = rng.integers(0, 3, N)
    sign = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    pts[out, ax[out]] = (sign * rng.uniform(1.05, 1.6, N) * h[ax])[out]
    faces = np.array([[a, b, c] for a in (-1, 0.25, 1) for b in (-1, -0.5, 1) for c in (-1, 0.125, 1)]) * h      # 27 points, 26 of them on a face
    k = min(len(faces), N)
    pts[:k] = faces[:k]
    if N > 4 * len(faces):
        pts[-len(faces):] = faces                 # again at the end: past the grid-stride cap in the big case
    return pts


def _ray_geometry(rng, R, G, half, faces_on):
    """Flat ray geometry for the voxel / grid kernels: points mostly inside the box of half-extents `half`, a sixth of them
    seen before the injection (t_M < 0 by a clear margin), and the last sample of every third
    ray exactly on an upper face of the box of half-extents `faces_on` with Omega = 0 (no rotation: the warped coordinate is the coordinate)."""
    P = R * G
    h = np.asarray(half, dtype=np.float64)
    c = rng.uniform(-0.9, 0.9, (3, P)) * h[:, None]
    far = rng.random(P) < 0.12                          # outside the grid at every rotation angle (the domain mask is an input)
    rad, ang = rng.uniform(1.5, 1.8, P) * max(faces_on[0], faces_on[1]), rng.uniform(0, 2 * np.pi, P)
    c[0, far], c[1, far] = (rad * np.cos(ang))[far], (rad * np.sin(ang))[far]
    Omega = rng.uniform(0.02, 0.3, P)
    t_geo = rng.uniform(0.5, 6.0, P)
    t_geo[rng.random(P) < 0.16] = -40.0                 # before the injection in every frame (t_M0 <= 20)
    fh = np.asarray(faces_on, dtype=np.float64)
    last = np.arange(R)[::3] * G + (G - 1)
    for j, p in enumerate(last):
        pt = rng.uniform(-0.5, 0.5, 3) * fh
        pt[j % 3] = fh[j % 3]                           # upper face of axis j % 3
        if j % 5 == 0:
            pt[:] = fh                                  # the upper corner
        c[:, p] = pt
        Omega[p] = 0.0
        t_geo[p] = 1.0
    return f32(c), f32(Omega), f32(t_geo)


def inputs(case):
    rng, p, fam = case.rng(), case.p, case.family
    if fam == 'geom':
        P, S = p['P'], p['S']
        rmin, rmax, zw = 3.0, 9.0, 8.0
        if p['exact']:
            # coordinates from small integers and powers of two: x^2 + y^2 + z^2 is exact in float32
            exact = np.array([[3, 0, 0], [0, 3, 0], [1, 2, 2], [2, 2, 1], [0, 0, 3], [9, 0, 0], [1, 4, 8], [4, 4, 7], [6, 6, 3], [8, 4, 1],
                              [7, 4, 4], [2, 1, 8], [0, 4, 8], [-4, -1, -8], [1, 2, -2], [-1, -4, -8], [-3, 0, 0], [0, -9, 0],
                              [2.5, 1.5, 0.5], [0.5, 0.5, 8], [1.5, 1.5, 2.0],
                              [2, 2, 0.5], [2, 2, 2], [9, 1, 0], [1, 4, 8.5], [0, 0, 2.75], [5, 5, 5], [4, 0, 8.25]], dtype=np.float64)
            c = np.tile(exact, (P // len(exact) + 1, 1))[:P].T.copy()
            c[:2, len(exact):] *= np.where(rng.random(P - len(exact)) < 0.5, -1.0, 1.0) if P > len(exact) else 1.0
        else:
            c = rng.uniform(-7.0, 7.0, (3, P))
            c[2] = rng.uniform(-9.5, 9.5, P)
            c32 = f32(c).astype(np.float64)
            r2 = (c32 ** 2).sum(0)
            near = lambda v, b: np.abs(v - b) <= 64 * 2.0 ** -23 * b
            tie = near(r2, rmin ** 2) | near(r2, rmax ** 2) | near(np.abs(c32[2]), zw)
            c[:, tie] = np.array([[4.0], [1.0], [2.0]])                   # off the tie: no point is excluded
            tail = np.arange(P) >= GEOM_CAP
            c[:, tail & (np.arange(P) % 2 == 0)] = np.array([[4.0], [-2.0], [1.0]])     # inside the domain, past the cap
        g, dtau, Sigma = (rng.uniform(0.5, 1.5, P) for _ in range(3))
        if P > GEOM_CAP:
            g[GEOM_CAP:] *= 2.0                                                # the largest weights where the second trip writes
        J = rng.uniform(-1.0, 1.0, (max(S, 1), P))
        return dict(coords=f32(c), g=f32(g), dtau=f32(dtau), Sigma=f32(Sigma), J=f32(J), rmin=rmin, rmax=rmax, z_width=zw)
    if fam == 'rt':
        N, R, G = p['N'], p['R'], p['G']
        e = rng.uniform(0.0, 1.0, (N, R, G))
        g, dtau, Sigma = (rng.uniform(0.5, 1.5, (R, G)) for _ in range(3))
        e[..., -1] = rng.uniform(2.0, 4.0, (N, R))          # the last sample carries weight: a dropped one shows even at G = 1024
        if G % 4:
            e[..., G - G % 4:] += 1.0
        dimg = rng.normal(size=(N, R))
        dimg[:, -1] = 3.0                                   # the last ray (tail of the last block) is not the smallest
        return dict(e=f32(e), g=f32(g), dtau=f32(dtau), Sigma=f32(Sigma), dimg=f32(dimg))
    if fam == 'chi2':
        B, S, R = p['B'], p['S'], p['R']
        if p['dtype'] == 'full':
            img, tgt, off = (rng.normal(size=(B, S, R)) for _ in range(3))
            sig = rng.uniform(0.5, 2.0, (B, S, R))
            img[..., R - (R % 4 or 1):] += 6.0              # tail elements and ...
            img[..., 1024:1040] += 5.0                      # ... the start of the second trip carry large residuals
            if B * S > LOSS_SUM_STRIDE:
                img.reshape(B * S, R)[LOSS_SUM_STRIDE:] += 4.0          # large terms where loss_sum_kernel strides
            return dict(images=f32(img), target=f32(tgt), sigma=f32(sig), offset=f32(off), scale=0.7)
        if p.get('cancel'):
            half = R // 2
            a = rng.uniform(0.5, 1.5, (B, S, half))
            img = np.zeros((B, S, R))
            img[..., :half] = a                              # a positive and a negative lobe (a Stokes Q / U image) ...
            img[..., half:2 * half] = -f32(a).astype(np.float64) * (1.0 - 2.0 ** -16)    # ... that cancel to 1.5e-5 of their size
            if R % 2:
                img[..., -1] = 0.05                         # the scalar tail element: a fifth of the whole light curve
            lc = f32(img).astype(np.float64).sum(-1)
            tgt, off = 0.4 * lc, 0.1 * lc
            sig = np.abs(lc) * rng.uniform(0.05, 0.2, (B, S))
        else:
            img = rng.normal(size=(B, S, R))
            img[..., R - (R % 4 or 1):] += 3.0
            tgt, off = rng.normal(size=(B, S)), 0.1 * rng.normal(size=(B, S))
            sig = rng.uniform(0.5, 2.0, (B, S))
            if B * S > LOSS_SUM_STRIDE:
                tgt.reshape(-1)[LOSS_SUM_STRIDE:] += 20.0
        return dict(images=f32(img), target=f32(tgt), sigma=f32(sig), offset=f32(off), scale=0.7)
    if fam == 'adam':
        n = p['n']
        par, g = rng.normal(size=n), rng.normal(size=n)
        if n > ADAM_CAP:
            g[ADAM_CAP:] *= 3.0
        if p.get('warm'):
            m, v = 0.3 * rng.normal(size=n), rng.uniform(0.1, 2.0, n)
        else:
            m, v = np.zeros(n), np.zeros(n)
        return dict(p=f32(par), g=f32(g), m=f32(m), v=f32(v), lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, gs=p['gs'], t=p['t'])
    if fam == 'eht':
        N, C_, nvis, R, dtype = p['N'], p['C'], p['nvis'], p['R'], p['dtype']
        RS = eht_splits(N * C_ * nvis, R)
        span = eht_span(R, RS)
        img = rng.uniform(0.2, 1.0, (N, R))
        big = 0.02 * R                                      # a pixel as bright as 2 % of the image: at the slice edges and the end
        marks = [R - 1] + [j * span + d for j in range(1, RS) for d in (-1, 0) if j * span < R]
        img[:, marks] = big
        if RS > 1:
            img[:, (RS - 1) * span:] *= 3.0                 # the last R-slice is the brightest
        if dtype == 'cphase':
            # coherent rows (a common phase per row, 30 % scatter): |vis| stays of the order of sum |a x|, the closure phase is well conditioned
            ph = rng.uniform(-np.pi, np.pi, (N, C_, nvis, 1))
            A = np.exp(1j * ph) * (1.0 + 0.3 * (rng.normal(size=(N, C_, nvis, R)) + 1j * rng.normal(size=(N, C_, nvis, R))))
            tgt = rng.uniform(-np.pi, np.pi, (N, nvis))
        else:
            A = rng.normal(size=(N, C_, nvis, R)) + 1j * rng.normal(size=(N, C_, nvis, R))      # both signs: the odd-R sums cancel
            vis = (A.astype(np.complex64).astype(np.complex128)[:, 0] @ f32(img).astype(np.float64)[:, :, None])[..., 0]
            noise = rng.normal(size=vis.shape) + 1j * rng.normal(size=vis.shape)
            tgt = 0.7 * vis + 0.2 * np.abs(vis).mean() * noise if dtype == 'vis' else 0.7 * np.abs(vis) + 0.1 * np.abs(vis).mean()
            if N * nvis > EHT_LOSS_BLOCK:
                flat = tgt.reshape(-1)
                flat[(N * nvis // EHT_LOSS_BLOCK) * EHT_LOSS_BLOCK:] *= 3.0       # the largest residuals in the last loss_part block
        sig = rng.uniform(0.5, 2.0, (N, nvis)) * (1.0 if dtype == 'cphase' else float(np.sqrt(R)))
        A = np.ascontiguousarray(A.astype(np.complex64))
        tgt = np.ascontiguousarray(tgt.astype(np.complex64)) if dtype == 'vis' else f32(tgt)
        return dict(images=f32(img), A=A, target=tgt, sigma=f32(sig), scale=0.5)
    if fam == 'trilinear':
        n, ext, N = p['n'], p['ext'], p['N']
        grid = smooth_grid(rng, n)
        pts = _points_in_box(rng, N, ext)
        if N > TRI_CAP:
            inside_tail = rng.uniform(-0.3, 0.3, (N - TRI_CAP - 27, 3)) * np.asarray(ext)
            pts[TRI_CAP:N - 27] = inside_tail
        return dict(points=f32(pts), grid=f32(grid), ext=f32(ext))
    if fam == 'voxel':
        B, R, G, S, n, ext = p['B'], p['R'], p['G'], p['S'], p['n'], p['ext']
        grids = np.stack([smooth_grid(rng, n) * (1.0 + 0.6 * b) for b in range(B)]) if p['per_frame'] else smooth_grid(rng, n)
        c, Omega, t_geo = _ray_geometry(rng, R, G, 0.5 * np.asarray(ext) * 0.7, faces_on=0.5 * np.asarray(ext))
        w = rng.uniform(0.5, 1.5, (max(S, 1), R * G)) * (np.where(rng.random((max(S, 1), 1)) < 0.5, -1.0, 1.0) if S else 1.0)
        w.reshape(max(S, 1), R, G)[..., -1] *= 3.0
        tM0 = np.linspace(2.0, 20.0, B)
        return dict(x=c[0], y=c[1], z=c[2], Omega=Omega, t_geo=t_geo, w=f32(w), tM0=f64(tM0), grid=f32(grids), ext=f32(ext))
    if fam == 'grid':
        B, R, G, S, res = p['B'], p['R'], p['G'], p['S'], p['res']
        scale = 4.0
        grid = smooth_grid(rng, (res,) * 3, lo=4.0, hi=14.0)           # sigmoid(grid - 10) spans 2e-3 .. 0.98
        c, Omega, t_geo = _ray_geometry(rng, R, G, (scale * 0.75,) * 3, faces_on=(scale,) * 3)
        dom = (rng.random(R * G) < 0.85).astype(np.uint8)
        dom.reshape(R, G)[::3, -1] = 1                                  # the upper-face samples are inside the domain
        w = rng.uniform(0.5, 1.5, (max(S, 1), R * G))
        w.reshape(max(S, 1), R, G)[..., -1] *= 3.0
        dimg = rng.normal(size=(B, max(S, 1), R))                       # signed: the gradient sums terms of both signs
        if S > 1:
            dimg[:, 1:] *= 2.0
        tM0 = np.linspace(2.0, 20.0, B)
        return dict(x=c[0], y=c[1], z=c[2], Omega=Omega, t_geo=t_geo, dom=dom, w=f32(w), tM0=f64(tM0), grid=f32(grid), scale=scale, dimg=f32(dimg))
    raise KeyError(fam)


# ===============================================================================================================
# references (float64 on the float32-rounded inputs) and their mutants
# ===============================================================================================================
MUTANTS = {
    'drop_last_sample': 'last sample of every ray dropped',
    'drop_tail4': 'last R % 4 / G % 4 elements dropped',
    'skip_second_block': 'rays / terms of the second block never computed',
    'skip_second_block_terms': 'chi^2 terms of the second loss_part block never added',
    'skip_second_trip': 'second grid-stride trip skipped: elements >= cap untouched',
    'skip_second_trip_r': 'second trip over the pixels skipped: pixels >= one trip untouched',
    'skip_second_trip_sum': 'loss_sum_kernel stops after its first 256 terms',
    'drop_last_slice': 'last R-slice of the EHT split dropped',
    'drop_last_element': 'span rounded down: the element past RS * span never summed',
    'dup_boundary': 'one element at a slice boundary counted twice',
    'closure_short': 'closure phase summed over C - 1 visibilities (loop bound off by one over C)',
    'frame0_grid': "frame 0's grid used for every frame",
    'swap_strides': 'ny / nz strides swapped',
    'one_extent': 'one extent used for all three axes',
    'stokes0': 'Stokes plane 0 used for every plane in the grid gradient',
    'upper_face_zero': 'upper-face points return 0',
    'exclusive_bounds': 'boundary comparisons made exclusive in the geometry fold',
    'bias_t_minus_1': 'Adam bias correction taken at t - 1',
    'ignore_grad_scale': 'grad_scale ignored',
    'f32_sum': "'lc' pixel sum accumulated in float32, in order",
}


def _swap_strides(grid):
    """The grid as a kernel would see it that indexes x*ny*nz + y*ny + z (ny where nz belongs)."""
    nx, ny, nz = grid.shape[-3:]
    X, Y, Z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
    idx = (X * ny * nz + Y * ny + Z) % (nx * ny * nz)
    flat = grid.reshape(grid.shape[:-3] + (-1,))
    return flat[..., idx]


def _on_upper_face(us, exts, ns):
    hit = np.zeros(np.shape(us[0]), dtype=bool)
    for u, f, n in zip(us, exts, ns):
        i = onp.world_to_index(u, float(f), n)
        hit |= (i == n - 1) & (n > 1)
    return hit


def reference(case, inp, mutant=None):
    p, fam = case.p, case.family
    assert mutant is None or mutant in MUTANTS
    if fam == 'geom':
        c = f64(inp['coords']); P = c.shape[1]
        r2 = (c ** 2).sum(0)
        rmin2, rmax2, zw = r32(inp['rmin']) ** 2, r32(inp['rmax']) ** 2, r32(inp['z_width'])
        if mutant == 'exclusive_bounds':
            dom = (r2 > rmin2) & (r2 < rmax2) & (np.abs(c[2]) < zw)
        else:
            dom = ~((r2 < rmin2) | (r2 > rmax2) | (np.abs(c[2]) > zw))
        w = f64(inp['g']) ** 2 * f64(inp['dtau']) * f64(inp['Sigma'])
        w = w[None] * f64(inp['J'])[:p['S']] if p['S'] else w[None]
        dom = dom.astype(np.float64)
        if mutant == 'skip_second_trip':
            w = w.copy(); w[:, GEOM_CAP:] = 0.0; dom = dom.copy(); dom[GEOM_CAP:] = 0.0
        return dict(w=w, dom=dom)
    if fam == 'rt':
        G, R = p['G'], p['R']
        w = f64(inp['g']) ** 2 * f64(inp['dtau']) * f64(inp['Sigma'])
        keep = np.ones(G)
        if mutant == 'drop_last_sample':
            keep[-1] = 0.0
        if mutant == 'drop_tail4':
            keep[G - G % 4:] = 0.0
        rays = np.ones(R)
        if mutant == 'skip_second_block':
            quads = (G + 3) // 4
            lpr = 1
            while lpr < 64 and lpr < quads:
                lpr *= 2
            rays[256 // lpr:] = 0.0
        img = (f64(inp['e']) * (w * keep)).sum(-1) * rays
        de = f64(inp['dimg'])[..., None] * (w * keep) * rays[:, None]
        return dict(img=img, de=de)
    if fam == 'chi2':
        B, S, R = p['B'], p['S'], p['R']
        img, tgt, sig, off, scale = f64(inp['images']), f64(inp['target']), f64(inp['sigma']), f64(inp['offset']), r32(inp['scale'])
        keep = np.ones(R)
        if mutant == 'drop_tail4':
            keep[R - R % 4:] = 0.0
        if mutant == 'skip_second_trip_r':
            keep[4096 if (R % 4 == 0 and not p['shift'] and not p['shift_out']) else 1024:] = 0.0
        if p['dtype'] == 'full':
            d = (img - tgt - off) / sig * keep
            planes = scale * (d ** 2).sum(-1).reshape(-1)
            dimg = 2.0 * scale * d / sig
        else:
            lc = (img * keep).sum(-1)
            if mutant == 'f32_sum':
                lc = np.cumsum(inp['images'].astype(np.float32), axis=-1, dtype=np.float32)[..., -1].astype(np.float64)
            d = (lc - tgt - off) / sig
            planes = (scale * d ** 2).reshape(-1)
            dimg = np.broadcast_to((2.0 * scale * d / sig)[..., None], img.shape).copy()
        loss0 = planes[:LOSS_SUM_STRIDE].sum() if mutant == 'skip_second_trip_sum' else planes.sum()
        out = dict(loss0=np.array(loss0), loss_planes=planes)
        if p['grad']:
            out['dimg'] = dimg
        return out
    if fam == 'adam':
        lr, b1, b2, eps, gs, t = r32(inp['lr']), r32(inp['b1']), r32(inp['b2']), r32(inp['eps']), r32(inp['gs']), int(inp['t'])
        g = f64(inp['g']) * (1.0 if mutant == 'ignore_grad_scale' else gs)
        tt = t - 1 if mutant == 'bias_t_minus_1' else t
        m = b1 * f64(inp['m']) + (1.0 - b1) * g
        v = b2 * f64(inp['v']) + (1.0 - b2) * g * g
        c1, c2 = r32(1.0 - b1 ** tt), r32(1.0 - b2 ** tt)         # the library rounds the two corrections to float (bhn_adam_hyper)
        par = f64(inp['p']) - lr * (m / c1) / (np.sqrt(v / c2) + eps)
        if mutant == 'skip_second_trip':
            par[ADAM_CAP:], m[ADAM_CAP:], v[ADAM_CAP:] = f64(inp['p'])[ADAM_CAP:], f64(inp['m'])[ADAM_CAP:], f64(inp['v'])[ADAM_CAP:]
        return dict(p=par, m=m, v=v)
    if fam == 'eht':
        return _eht_reference(case, inp, mutant)
    if fam == 'trilinear':
        grid, ext, pts = f64(inp['grid']), [float(v) for v in inp['ext']], f64(inp['points'])
        if mutant == 'swap_strides':
            grid = _swap_strides(grid)
        if mutant == 'one_extent':
            ext = [ext[0]] * 3
        out = onp.trilinear_world(grid, ext, pts[:, 0], pts[:, 1], pts[:, 2])
        if mutant == 'upper_face_zero':
            out = np.where(_on_upper_face(pts.T, ext, grid.shape), 0.0, out)
        if mutant == 'skip_second_trip':
            out[TRI_CAP:] = 0.0
        return dict(out=out)
    if fam == 'voxel':
        B, R, G, S = p['B'], p['R'], p['G'], p['S']
        grid, ext = f64(inp['grid']), [float(v) for v in inp['ext']]
        if mutant == 'frame0_grid':
            grid = np.broadcast_to(grid[:1], grid.shape)
        if mutant == 'swap_strides':
            grid = _swap_strides(grid)
        if mutant == 'one_extent':
            ext = [ext[0]] * 3
        geo = [inp[k] for k in ('x', 'y', 'z', 'Omega', 't_geo')]
        images, e = onp.voxel_render(grid, ext, *geo, inp['tM0'], inp['w'], R, G)
        if mutant == 'upper_face_zero':
            ux, uy, uz, _ = onp.warp_points(*geo, inp['tM0'])
            e = np.where(_on_upper_face((ux, uy, uz), ext, grid.shape[-3:]), 0.0, e)
        if mutant == 'drop_last_sample':
            e = e.reshape(B, R, G).copy(); e[..., -1] = 0.0; e = e.reshape(B, R * G)
        return dict(images=onp.render_weighted(e, inp['w'], R, G))
    if fam == 'grid':
        return _grid_reference(case, inp, mutant, absolute=False)
    raise KeyError(fam)


def _grid_reference(case, inp, mutant, absolute):
    p = case.p
    B, R, G, S, res = p['B'], p['R'], p['G'], p['S'], p['res']
    grid, scale = f64(inp['grid']), r32(inp['scale'])
    geo = [inp[k] for k in ('x', 'y', 'z', 'Omega', 't_geo')]
    e, (ux, uy, uz, live) = onp.grid_emission(grid, scale, *geo, inp['tM0'], inp['dom'])
    dimg, w, dom = f64(inp['dimg']), f64(inp['w']), inp['dom']
    if absolute:
        dimg, w = np.abs(dimg), np.abs(w)
    if mutant == 'stokes0':
        dimg = np.broadcast_to(dimg[:, :1], dimg.shape)
    if mutant == 'upper_face_zero':
        face = _on_upper_face((ux, uy, uz), (2 * scale,) * 3, (res,) * 3) & live
        e = np.where(face, onp.sigmoid(-10.0), e)
        dom = np.where(face.any(0), 0, dom)              # ... and send no gradient through these samples
    if mutant == 'drop_last_sample':
        e = e.reshape(B, R, G).copy(); e[..., -1] = 0.0; e = e.reshape(B, R * G)
        dom = np.asarray(dom).reshape(R, G).copy(); dom[:, -1] = 0; dom = dom.reshape(-1)
    dgrid = onp.grid_render_grad(grid, scale, *geo, inp['tM0'], dom, w, dimg, R, G)
    return dict(emission=e, images=onp.render_weighted(e, w, R, G), dgrid=dgrid)


def _eht_reference(case, inp, mutant):
    """loss_fn_eht (network.py:541-564) and its gradient w.r.t. the images, written out."""
    p = case.p
    N, C_, nvis, R, dtype = p['N'], p['C'], p['nvis'], p['R'], p['dtype']
    RS = eht_splits(N * C_ * nvis, R)
    span = eht_span(R, RS)
    A = inp['A'].astype(np.complex128).reshape(N, C_, nvis, R)
    x, sig, scale = f64(inp['images']), f64(inp['sigma']), r32(inp['scale'])
    wr = np.ones(R)
    if mutant == 'drop_last_slice':
        wr[(RS - 1) * span:] = 0.0
    if mutant == 'drop_last_element':
        wr[RS * ((R // RS) & ~1) if RS > 1 else R - 1:] = 0.0
    if mutant == 'dup_boundary':
        wr[span] = 2.0
    vis = (A * (x * wr)[:, None, None, :]).sum(-1)                 # (N, C, nvis)
    if dtype == 'vis':
        d = vis[:, 0] - inp['target'].astype(np.complex128)
        terms = np.abs(d) ** 2 / sig ** 2
        gv = (2.0 * scale * d / sig ** 2)[:, None]
    elif dtype == 'amp':
        amp = np.abs(vis[:, 0])
        d = (amp - f64(inp['target'])) / sig
        terms = d ** 2
        gv = ((2.0 * scale * d / (sig * amp)) * vis[:, 0])[:, None]
    else:
        used = np.ones(C_)
        if mutant == 'closure_short':
            used[-1] = 0.0
        phi = (np.angle(vis) * used[None, :, None]).sum(1)
        d = f64(inp['target']) - phi
        terms = (1.0 - np.cos(d)) / sig ** 2
        dphi = -scale * np.sin(d) / sig ** 2
        gv = dphi[:, None] * (-vis.imag + 1j * vis.real) / np.abs(vis) ** 2 * used[None, :, None]
    flat = terms.reshape(-1)
    if mutant == 'skip_second_block_terms':
        flat = flat[:EHT_LOSS_BLOCK]
    if mutant == 'skip_second_trip_sum':
        flat = flat[:LOSS_SUM_STRIDE * EHT_LOSS_BLOCK]
    out = dict(loss0=np.array(scale * flat.sum()))
    if p.get('grad', True):
        out['dimg'] = (gv.real[..., None] * A.real + gv.imag[..., None] * A.imag).sum((1, 2))
    return out


# ===============================================================================================================
# scales and the comparator
# ===============================================================================================================
def scales(case, inp, ref):
    """Denominators: the largest entry of the reference, as the existing tests measure each kernel -- except the grid
    gradient (signed dimages scattered into shared voxels), where it is the largest entry of the reference evaluated on
    |dimages| and |w|."""
    sc = {k: float(np.abs(v).max()) for k, v in ref.items() if not k.startswith('_')}
    if case.family == 'grid':
        sc['dgrid'] = float(np.abs(_grid_reference(case, inp, None, absolute=True)['dgrid']).max())
    if case.family == 'geom':
        sc['dom'] = 1.0
    return sc


def errors(case, got, ref, sc):
    """name -> (observed, bound).  `got` holds the same keys as the reference (minus the private ones)."""
    out = {}
    for k, r in ref.items():
        if k.startswith('_'):
            continue
        g = np.asarray(got[k], dtype=np.float64).reshape(np.shape(r))
        b = case.bounds[k]
        if b == 0.0:
            out[k] = (float((g != r).sum()), 0.0)
        else:
            out[k] = (float(np.abs(g - r).max()) / sc[k], b)
    return out


def worst(errs):
    """Largest observed / bound over the outputs (an exact output that differs counts as infinitely over)."""
    return max((np.inf if o > 0 else 0.0) if b == 0.0 else o / b for o, b in errs.values())


def report(case, errs):
    return '%s: ' % case.id + ', '.join('%s %.2e / %.0e' % (k, o, b) for k, (o, b) in errs.items())
