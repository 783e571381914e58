"""The case table of bhn_volume_render (bhnerf_amd/csrc/volume_render.hip), shared by tests/test_gpu_volume.py (runs each case
on the device) and tests/test_volume_refs_cpu.py (proves on the CPU that the restatement below is the reference's arithmetic, and
that each case sees the slips it is for).  NumPy only; the pattern of tests/standalone_cases.py.

`render_ref` restates VolumeVisualizer.render from its description (colour and alpha -> wireframe -> black hole -> clip ->
colour x step of image row 0 -> mask -> back-to-front composite), in any float dtype; tests/test_volume_refs_cpu.py holds it to
the images the reference's own code produced (tests/golden/g13_volume.npz) at 1e-12.

A case is (name, parameters, `why`, mutants).  inputs(case) -> float32 arrays + the view; reference(case, inp[, mutant]) ->
float64 images (N, H, W, 3) from the float32-rounded inputs; errors are the largest absolute difference over the largest entry of
the reference, as standalone_cases.BOUNDS measures every other kernel.
"""
import os
import zlib

import numpy as np

SENTINEL = -777.25
GUARD = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g13_volume.npz')

# BOUND: largest |kernel - float64 restatement| / largest reference entry.  Measured on the MI355X over the whole table (per case
# in DESIGN.md 4.8): 2.0e-7 at the worst (golden_b); 4 x that, rounded up to one digit, is 8e-7.  But the bound may not be under the
# float32 floor of the restatement itself -- render_ref in float32 against float64 on the same float32 inputs, on the CPU: up to
# 1.39e-6 on these cases (golden_b; test_volume_refs_cpu.py asserts it) -- which is what single precision costs the reference's own
# arithmetic; rounded up to one digit that is the bound.  (The kernel sits under the floor because it forms the wireframe
# distances, where float cancellation costs the most, in double.)
BOUND = 2e-6
MUTANT_FACTOR = 5.0

f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
r32 = lambda v: float(np.float32(v))


# ===============================================================================================================
# the restatement
# ===============================================================================================================
def wire_points(fw, dtype=np.float64, stubs=True):
    """The (i, j, k) wireframe points q = v_i + t_k d_j: (n, 64, 3).  stubs=False leaves out the 24 segments that point away
    from the cube (d_j along the sign of the vertex coordinate)."""
    h = dtype(fw) / dtype(2)
    t = np.linspace(0.0, float(fw), 64).astype(dtype)
    segs = []
    for i in range(8):
        v = np.array([h if i & 1 else -h, h if i & 2 else -h, h if i & 4 else -h], dtype=dtype)
        for j in range(6):
            d = np.zeros(3, dtype=dtype)
            d[j // 2] = 1.0 if j & 1 else -1.0
            if not stubs and d[j // 2] * v[j // 2] > 0:
                continue
            segs.append(v[None, :] + t[:, None] * d[None, :])
    return np.stack(segs)


def wire_alpha(pts, fw, lw, dtype=np.float64, stubs=True):
    """1e6 sum_q exp(-|p - q| / lw^2) at every point, segment by segment in the reference's order."""
    p = np.asarray(pts, dtype=dtype).reshape(-1, 3)
    out = np.zeros(len(p), dtype=dtype)
    lw2 = dtype(lw) ** 2
    for seg in wire_points(fw, dtype, stubs):
        dist = np.sqrt(((p[:, None, :] - seg[None, :, :]) ** 2).sum(-1))
        term = dtype(1e6) * np.exp(-dist / lw2)
        for k in range(term.shape[1]):
            out += term[:, k]
    return out.reshape(np.shape(pts)[:-1])


def render_ref(pts, emission, alpha_scale, lut, fw, lw, bh_radius, albedo, dtype=np.float64, mutant=None, wire=None):
    """Images (N, H, W, 3).  pts (H, W, S, 3), emission (N, H, W, S), alpha_scale (N), lut (n, 3).  `wire`: a precomputed
    wire_alpha(pts, fw, lw, dtype) (it does not depend on the frame)."""
    assert mutant is None or mutant in MUTANTS, mutant
    T = dtype
    p = np.asarray(pts, dtype=T)
    e = np.asarray(emission, dtype=T)
    lut = np.asarray(lut, dtype=T)
    n = len(lut)
    H, W, S = p.shape[:3]
    fw, lw, bh = T(fw), T(lw), T(bh_radius)
    if mutant == 'frame0_emission':
        e = np.broadcast_to(e[:1], e.shape)
    sc = np.asarray(alpha_scale, dtype=T)
    if mutant == 'frame0_scale':
        sc = np.broadcast_to(sc[:1], sc.shape)
    # 1. colour and alpha
    x = e * T(n)
    idx = np.where(x == n, n - 1, np.trunc(np.clip(x, -1, n))).astype(np.int64)
    if mutant == 'equal_wraps':
        idx = np.where(x >= n, 0, idx)
    idx = np.clip(idx, 0, n - 1)
    rgb = np.clip(lut[idx] - (T(0) if mutant == 'no_minus_005' else T(0.05)), 0, 1)
    a = e * sc[:, None, None, None]
    # 2. wireframe
    if wire is None or mutant == 'no_stubs':
        wire = wire_alpha(p, fw, lw, T, stubs=mutant != 'no_stubs')
    a = a + wire[None]
    amax = np.abs(p).max(-1)
    zero = amax > fw / T(2) + lw
    if mutant != 'no_zero_mask':
        a = np.where(zero[None], 0, a)
        rgb = np.where(zero[None, ..., None], 0, rgb)
    # 3. black hole
    norm = np.sqrt((p ** 2).sum(-1))
    if bh > 0 and mutant != 'bh_ignored':
        light = np.array([-1.0, -1.0, 1.0], dtype=T) / np.sqrt(T(3))
        shade = (p * light).sum(-1)[..., None] * np.asarray(albedo, dtype=T)
        hole = norm < bh
        rgb = np.where(hole[None, ..., None], shade[None], rgb)
        a = np.where(hole[None], 1, a)
    # 4. clip
    rgb = np.clip(rgb, 0, 1)
    if mutant != 'alpha_unclipped':
        a = np.clip(a, 0, 1)
    # 5. colour x step (of image row 0)
    step = np.zeros((H, W, S), dtype=T)
    step[..., :-1] = np.sqrt(((p[:, :, 1:] - p[:, :, :-1]) ** 2).sum(-1))
    if mutant != 'step_row_h':
        step = np.broadcast_to(step[:1], step.shape)
    color = rgb * step[None, ..., None]
    # 6. mask
    m = ((amax < fw / T(2) - lw) & (norm > (T(0) if mutant == 'bh_ignored' else bh))).astype(T)
    # 7. composite, back to front
    R = np.zeros(e.shape[:3] + (3,), dtype=T)
    acc = np.zeros(e.shape[:3], dtype=T)
    order = range(S) if mutant == 'front_to_back' else range(S - 1, -1, -1)
    if mutant == 'drop_tail_chunk' and S > 64:
        order = [s for s in order if s < 64 * ((S - 1) // 64)]
    held = np.zeros_like(R)
    for s in order:
        if mutant == 'chunk_carry_lost' and s % 64 == 63 and s != S - 1:
            # what is behind a 64-sample chunk boundary is added un-attenuated by the chunks in front of it
            held, R = held + R, np.zeros_like(R)
        c, ms, as_ = color[:, :, :, s], m[None, :, :, s], a[:, :, :, s]
        R = R + ms[..., None] * c
        oa = as_ * (1 - ms)
        R = R * (1 - oa[..., None]) + c * oa[..., None]
        acc = as_ + (1 - as_) * acc
    R = R + held
    if mutant != 'no_background':
        R = R + (1 - acc)[..., None]
    return R


MUTANTS = {
    'step_row_h': "step length taken from the ray's own image row instead of row 0",
    'front_to_back': 'composited front to back',
    'no_background': 'white background term dropped',
    'no_minus_005': 'the - 0.05 on the colours dropped',
    'bh_ignored': 'black hole ignored',
    'no_zero_mask': 'points outside facewidth/2 + linewidth not zeroed',
    'no_stubs': 'the 24 outward stubs of the wireframe dropped',
    'chunk_carry_lost': 'prefix product restarts at every 64-sample chunk',
    'drop_tail_chunk': 'the last (partial or whole) 64-sample chunk of a ray dropped',
    'frame0_emission': "frame 0's emission rendered for every frame",
    'frame0_scale': "frame 0's alpha scale used for every frame",
    'equal_wraps': 'e lut_n >= lut_n wraps to entry 0 instead of the last entry',
    'alpha_unclipped': 'alpha not clipped to [0, 1]',
}


# ===============================================================================================================
# the table
# ===============================================================================================================
class Case:
    def __init__(self, name, why, mutants, **p):
        self.name, self.why, self.mutants = name, why, tuple(mutants)
        self.p = dict(H=4, W=5, S=16, N=1, pad=0, fw=3.8, lw=0.1, bh=0.0, albedo=(0.0, 0.0, 0.0), lut_n=256, shift=0, cam=(9.0, 2.0, 0.7, 1.0), trange=None,
                      kind='camera', e_kind='smooth')
        self.p.update(p)
        self.id = 'volume-' + name

    def __repr__(self):
        return self.id

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.id.encode()))


def _cases():
    C = []
    add = lambda *a, **k: C.append(Case(*a, **k))
    common = ('step_row_h', 'front_to_back', 'no_background', 'no_minus_005')
    add('golden_a', 'golden view a, 12 x 10 x 70 (two chunks: 64 + 6), no black hole', common + ('no_zero_mask',), kind='golden', view='a')
    add('golden_a_bh', 'golden view a with the black hole, albedo (0.9, 0.6, 0.3)', ('bh_ignored', 'front_to_back'), kind='golden', view='a', bh=2.0, albedo=(0.9, 0.6, 0.3))
    add('golden_b', 'golden view b, 24 x 16 x 33 (LPR = 64 with 31 idle lanes), no black hole', common + ('no_zero_mask',), kind='golden', view='b')
    add('golden_b_bh', 'golden view b with the black hole', ('bh_ignored', 'no_background'), kind='golden', view='b', bh=2.0, albedo=(0.9, 0.6, 0.3))
    add('stub_vertex', 'hand-placed points: a sample within linewidth of a cube vertex and outside the cube, where only the outward stubs reach alpha 1',
        ('no_stubs',), kind='stub', H=1, W=2, S=3, fw=2.0)
    add('S1', 'S = 1: one sample, step 0: the image is the background term alone', ('no_background',), H=3, W=4, S=1)
    add('S2', 'S = 2: LPR = 16, one live step; both samples inside the cube', ('no_minus_005', 'no_background', 'step_row_h'), H=3, W=4, S=2, trange=(-1.0, 1.0))
    add('S20_lpr32', 'S = 20: LPR = 32, W != H, 35 rays: the last block has 3 of its 8 rays', common, H=5, W=7, S=20)
    add('S63', 'S = 63: one chunk, one idle lane', ('front_to_back', 'no_zero_mask'), H=2, W=3, S=63)
    add('S64', 'S = 64: exactly one chunk', ('front_to_back', 'no_zero_mask'), H=2, W=3, S=64)
    add('S65', 'S = 65: a second chunk of one sample, which lies inside the cube behind the shell and the wires (its own colour is 0: the last step is)', ('drop_tail_chunk',), H=2, W=3, S=65, trange=(-4.0, 1.5), cam=(9.0, 0.5, 0.7, 1.0), e_kind='sparse')
    add('S130', 'S = 130: three chunks, the last two samples inside the cube', ('chunk_carry_lost', 'drop_tail_chunk'), H=2, W=3, S=130, trange=(-4.0, 1.5), cam=(9.0, 0.5, 0.7, 1.0), e_kind='sparse')
    add('one_ray', 'H W = 1: one ray, one live group of one block', ('front_to_back', 'no_minus_005'), H=1, W=1, S=40, cam=(9.0, 2.0, 0.7, 1.0))
    add('H1', 'H = 1: row 0 is the only row', ('front_to_back', 'no_minus_005'), H=1, W=9, S=16)
    add('N3_padded', 'N = 3 frames, frame_stride padded by 37 floats, each frame its own alpha scale', ('frame0_emission', 'frame0_scale'), N=3, pad=37, H=3, W=5, S=33)
    add('N6_two_groups', 'N = 6 frames: two frame groups of the launch (4 + 2)', ('frame0_emission', 'frame0_scale'), N=6, H=2, W=3, S=16)
    add('miss', 'every ray misses the cube: the image is exactly (1, 1, 1)', ('no_zero_mask',), kind='miss', H=3, W=3, S=16, exact_one=True)
    add('e_edges', 'e exactly 0, exactly 1, slightly above 1 and negative, inside the cube; lut_n = 256', ('equal_wraps', 'alpha_unclipped'), e_kind='edges', H=3, W=4, S=16)
    add('lut2', 'lut_n = 2, e on both sides of 0.5 and exactly 1', ('equal_wraps', 'no_minus_005'), e_kind='edges', lut_n=2, H=3, W=4, S=16)
    add('shell', 'samples in the shell facewidth/2 - lw < max|p_c| < facewidth/2 + lw, on and off the wires: neither zeroed nor inside',
        ('no_zero_mask', 'front_to_back'), kind='shell', H=2, W=4, S=16)
    add('bh_both_signs', 'black hole with l . p of both signs (camera on the lit side sees the dark limb too), albedo (1, 0.5, 0.25)', ('bh_ignored',),
        bh=1.2, albedo=(1.0, 0.5, 0.25), H=6, W=6, S=33, cam=(9.0, 2.0, 2.5, 1.2))
    add('misaligned', 'every input and the output on 4-byte aligned sub-views', ('front_to_back',), shift=1, H=3, W=5, S=20)
    return C


CASES = _cases()
REFUSALS = ['null_pts', 'null_emission', 'null_scale', 'null_lut', 'null_view', 'null_images', 'N0', 'H0', 'W0', 'S0', 'lut_n1', 'facewidth0', 'linewidth0',
            'bh_negative']


# ===============================================================================================================
# inputs
# ===============================================================================================================
def camera_points(H, W, S, cam_r, domain_r, azimuth, zenith, trange=None):
    """A pinhole camera at cam_r looking at the origin, S samples per ray across the domain: float64 (H, W, S, 3)."""
    o = cam_r * np.array([np.cos(azimuth) * np.sin(zenith), np.sin(azimuth) * np.sin(zenith), np.cos(zenith)])
    fwd = -o / np.linalg.norm(o)
    right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    half = np.tan(1.06 * np.arctan(np.sqrt(3) * domain_r / cam_r))
    u = (np.arange(W) + 0.5 - W / 2) / (W / 2) * half
    v = -(np.arange(H) + 0.5 - H / 2) / (W / 2) * half
    d = fwd[None, None] + u[None, :, None] * right[None, None] + v[:, None, None] * up[None, None]
    lo, hi = trange if trange is not None else (-np.sqrt(3) * domain_r, np.sqrt(3) * domain_r)
    t = np.linspace(cam_r + lo, cam_r + hi, S)
    return o[None, None, None] + t[None, None, :, None] * d[:, :, None, :]


def golden():
    g = dict(np.load(GOLDEN))
    return g


def inputs(case):
    p, rng = case.p, case.rng()
    H, W, S, N = p['H'], p['W'], p['S'], p['N']
    fw, lw = p['fw'], p['lw']
    if p['kind'] == 'golden':
        g = golden()
        pts, e = g['pts_' + p['view']], g['emission_' + p['view']][None]
        H, W, S = pts.shape[:3]
        fw, lw = float(g['params'][2]), float(g['params'][3])
        lut = g['lut_hot']
    else:
        cam_r, dom_r, az, zen = p['cam']
        pts = camera_points(H, W, S, cam_r, dom_r, az, zen, p['trange'])
        h = fw / 2
        if p['kind'] == 'miss':
            pts = pts + np.array([40.0, 0.0, 0.0])
        if p['kind'] == 'stub':
            q = np.array([1.098, 1.098, 1.098])
            pts = np.zeros((1, 2, 3, 3))
            pts[0, 0] = [q + [2.0, 0.0, 0.0], q, q - [3.0, 0.0, 0.0]]               # ray 0: outside, at the vertex, outside
            pts[0, 1] = [[0.2, 0.1, -2.0], [0.2, 0.1, 0.0], [0.2, 0.1, 2.0]]         # ray 1: through the middle of the cube
        if p['kind'] == 'shell':
            k = S // 2
            for w in range(W):                      # sample k of every ray of both rows: in the shell, w = 0, 1 on an edge line
                s = h + (0.06 if w % 2 else -0.06)
                pts[:, w, k] = [[s, s, 0.3 * h] if w < 2 else [s, 0.4 * h, -0.2 * h]] * H
        x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
        blob = np.exp(-((x - 0.5) ** 2 + (y + 0.3) ** 2 + (z - 0.2) ** 2) / (2 * 0.8 ** 2))
        e = np.stack([np.clip(0.02 + (0.9 - 0.12 * n) * np.roll(blob, n, axis=1) + 0.05 * rng.uniform(size=blob.shape), 0, 0.999) for n in range(N)])
        if p['e_kind'] == 'sparse':
            # few emitting samples, so that the background product survives a long ray: four inside the cube (the last two of the
            # ray among them), every sample of the shell, and one bright sample in the zeroed region that sets the alpha scale
            amax = np.abs(pts).max(-1)
            e = np.zeros_like(e)
            e[..., [S // 4, S // 2, S - 2, S - 1]] = 0.6
            e[:, (amax > h - lw) & (amax < h + lw)] = 0.4
            e[..., 0] = 2.0
            assert (amax[..., 0] > h + lw).all() and (amax[..., S - 2:] < h - lw).all()
        if p['e_kind'] == 'edges':
            inside = np.abs(pts).max(-1) < h - lw
            vals = np.array([0.0, 1.0, 1.0 + 2.0 ** -20, -0.25, 0.49, 0.51, 1.5, -2.0 ** -30])
            flat, where = e.reshape(-1), np.flatnonzero(inside.reshape(-1))
            assert len(where) >= 2 * len(vals)
            flat[where[:2 * len(vals)]] = np.tile(vals, 2)
            outside = np.flatnonzero(~inside.reshape(-1))
            flat[outside[::3]] = -0.4                                                # negative alpha outside the inside region, near the wires too
        n = p['lut_n']
        t = np.linspace(0.0, 1.0, n)[:, None]
        lut = np.clip(np.concatenate([0.04 + 2.4 * t, 1.9 * t - 0.5, 3.0 * t - 2.0], axis=1), 0, 1) if n > 2 else np.array([[0.1, 0.3, 0.9], [1.0, 0.8, 0.2]])
    e32 = f32(e)
    amax = e32.reshape(len(e32), -1).max(1)
    scale = (np.float32(1.0) / amax).astype(np.float32)
    return dict(pts=f32(pts), emission=e32, alpha_scale=scale, lut=f32(lut), fw=float(fw), lw=float(lw), bh=float(p['bh']), albedo=tuple(float(a) for a in p['albedo']),
                H=H, W=W, S=S, N=len(e32))


def reference(case, inp, mutant=None, dtype=np.float64, wire=None):
    return render_ref(inp['pts'], inp['emission'], inp['alpha_scale'], inp['lut'], inp['fw'], inp['lw'], inp['bh'], inp['albedo'], dtype=dtype, mutant=mutant, wire=wire)


def error(got, ref):
    """Largest absolute difference over the largest entry of the reference."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def report(case, err):
    return '%s: %.2e / %.0e' % (case.id, err, BOUND)
