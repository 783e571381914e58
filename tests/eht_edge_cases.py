"""The edge-shape table of the (u, v) EHT kernels -- csrc/eht_uv_kernels.h, compiled into libbhnerf_eht.so, libbhnerf_cls.so and
libbhnerf_pol.so, and the loss kernels of csrc/eht_uv.hip, eht_closure.hip and eht_pol.hip -- shared by
tests/test_eht_edge_cases_cpu.py (proves on the CPU that each case's bound sees the slips the case is for) and
tests/test_gpu_eht_edges.py (runs each case on the device).  NumPy and torch on the CPU only.

Built on eht_uv_cases.py, closure_cases.py and pol_cases.py: their generators through the explicit (H, W, B, seed, stations) of
case(), in their documented order of draws, their float64 references (table_loss, closure_loss, pol_loss) and their bounds.
Nothing here is fitted to a device: a seed is the smallest at which the float64 reference meets the admission conditions in every
form of the case and, for 'turns', at which its mutant shows in all three outputs (tests/test_eht_edge_cases_cpu.py).

A case names the line of a kernel it is for (`why`), the plan values that claim rests on (`claims`, asserted against plan(),
which restates eht_make_plan; the CPU test holds the restatement to a C++ build of csrc/eht_uv.h) and the slips it must catch
(`mutants`: MUTANTS).  A mutant is built into the float64 reference, never into a kernel.

Admission (asserted in admitted()): a case that carries 'cphase' or 'logcamp' has smallest |vis| / largest |vis| >= MIN_AMP;
a pol case has smallest |I| / largest |I| >= MIN_AMP (pol_cases.case asserts it).  'turns' carries 'vis' and 'amp' only: a
resolved-out baseline is the point of that case.  'n260' is 16 x 16 pixels, not 8 x 8: at 8 x 8 the blob is narrower than a
pixel, the 5 % noise carries most of the flux, and no seed below 1500 keeps all 1560 visibilities of 260 random arrays above
MIN_AMP (best 0.047); with the blob resolved by the grid, seed 8 does.  The pol form of 'n260' (B 257, 8 x 8) is admitted as it
stands.  'turns' has a field of view of 10000 x FOV, not 200 x: at 200 x (237 turns) a float32 phase moves the visibilities by
1.9e-5 of the largest, less than the bound itself, so that input could not see the slip it is for; at 10000 x (some 12000 turns)
it moves visibilities, loss and dimages by 1e-3 and more."""
import numpy as np

import closure_cases as K
import eht_uv_cases as E
import pol_cases as P

# ---- the constants of the kernels the shapes are chosen from (csrc/eht_uv.h)
EHT_KB, EHT_MIN_ROWS, EHT_MAX_SPLITS, EHT_ADJ_ROWS, WAVE, LANES = 8, 8, 64, 4, 64, 256

# The bounds of test_gpu_closure.py for figures that hold 'logcamp' (its LOGCAMP_BOUND; both test modules assert the identity).
CLS_LOGCAMP_BOUND = {'loss': 1.2e-5, 'dimages': 2.8e-5}
CLS_DTYPE, CLS_SCALE = 'amp+cphase+logcamp', 2.0          # the full combined dtype at closure_cases.WEIGHTS, the siblings' scale
POL_DTYPE = 'pvis+m'


def plan(N, nvis, H, W):
    """eht_make_plan and eht_row_splits restated, with what the launches make of them: `trips` of the column loop of
    eht_fwd_kernel, `col_blocks` and `strips` of eht_adjoint_kernel's grid, `last_live` lanes of the last column trip (= of the
    last column block), `tail_lanes` of them in its last wave, `last_rows` of the last row split."""
    kblocks = (nvis + EHT_KB - 1) // EHT_KB
    rs = (256 + kblocks - 1) // kblocks
    rs = max(1, min(rs, (H + EHT_MIN_ROWS - 1) // EHT_MIN_ROWS, EHT_MAX_SPLITS))
    rows_per = (H + rs - 1) // rs
    RS = (H + rows_per - 1) // rows_per
    rows_per = (H + RS - 1) // RS
    block = WAVE * max(1, min(4, (W + WAVE - 1) // WAVE))
    trips = (W + block - 1) // block
    last_live = W - (trips - 1) * block
    return dict(N=N, nvis=nvis, H=H, W=W, kblocks=kblocks, RS=RS, rows_per=rows_per, block=block, waves=block // WAVE, trips=trips,
                col_blocks=trips, last_live=last_live, tail_lanes=last_live - WAVE * ((last_live - 1) // WAVE), strips=(H + EHT_ADJ_ROWS - 1) // EHT_ADJ_ROWS,
                last_rows=H - (RS - 1) * rows_per)


MUTANTS = {   # slip -> the outputs it changes
    'first_wave_only': ('vis', 'loss', 'dimages'),           # columns with (x mod block) >= 64 contribute nothing to the visibilities
    'first_trip_only': ('vis', 'loss', 'dimages'),           # columns x >= 256 contribute nothing
    'adjoint_first_block_only': ('dimages',),                # dimages columns >= 256 are zero
    'first_256_baselines': ('loss', 'dimages'),              # entries >= 256 of every per-plane list a 256-lane loop strides over
                                                             # (baselines, triangles, quadrangles) are dropped from loss and gradient
    'first_256_planes': ('loss',),                           # planes (pol: frames) >= 256 are dropped from the loss
    'last_split_dropped': ('vis', 'loss', 'dimages'),        # rows of the last row split contribute nothing
    'float32_phase': ('vis', 'loss', 'dimages'),             # the twiddle phase is formed in float32
}


class Case:
    """spec (H, W, B, seed, stations); uv: the dtypes libbhnerf_eht.so runs; uv_Sx / cls_Sx: the Stokes axes (0: none) it is run
    with there; pol: (spec, Sx...) or None."""

    def __init__(self, name, spec, why, mutants, claims, uv=('vis', 'amp', 'cphase'), uv_Sx=(0,), cls_Sx=(), pol=None, fov=E.FOV):
        self.name, self.spec, self.why, self.mutants, self.claims = name, tuple(spec), why, tuple(mutants), claims
        self.uv, self.uv_Sx, self.cls_Sx, self.pol, self.fov = tuple(uv), tuple(uv_Sx), tuple(cls_Sx), pol, fov
        self.H, self.W, self.B, self.seed, self.ns = self.spec
        self.nvis = self.ns * (self.ns - 1) // 2
        self.ncp = self.ns * (self.ns - 1) * (self.ns - 2) // 6
        self.nca = 2 * (self.ns * (self.ns - 1) * (self.ns - 2) * (self.ns - 3) // 24)
        assert all(m in MUTANTS for m in self.mutants), name
        got = dict(plan(self.B, self.nvis, self.H, self.W), ncp=self.ncp, nca=self.nca)
        assert all(got[k] == v for k, v in claims.items()), (name, claims, got)       # the plan values `why` claims

    def __repr__(self):
        return self.name


def _cases():
    C = []
    add = lambda *a, **k: C.append(Case(*a, **k))
    fwd = ('first_wave_only',)
    add('w65', (5, 65, 1, 0, 4), 'eht_fwd_kernel: block 128, red[j][1] of a second wave with one live lane enters `for (w = 1; w < waves; ++w)`',
        fwd, dict(block=128, waves=2, trips=1, last_live=65, tail_lanes=1, RS=1))
    add('w130', (9, 130, 1, 0, 5), 'eht_fwd_kernel: block 192, three waves in the red[j][w] sum, the third with 2 live lanes; the shared kernels in '
        'the closure and pol builds', fwd, dict(block=192, waves=3, trips=1, tail_lanes=2, RS=2, rows_per=5, last_rows=4), cls_Sx=(0,), pol=((9, 130, 1, 0, 5), 3))
    add('w256', (4, 256, 1, 0, 4), 'eht_fwd_kernel: block 256, four full waves, one trip of `x += blockDim.x`', fwd,
        dict(block=256, waves=4, trips=1, last_live=256, strips=1))
    add('w300', (7, 300, 2, 0, 5), 'eht_fwd_kernel: second trip of `for (x = threadIdx.x; x < W; x += blockDim.x)`; eht_adjoint_kernel: blockIdx.x = 1 '
        'with 44 live lanes, the others leave at `if (x >= p.W) return`; H % 4 = 3: the strip rows past H', fwd + ('first_trip_only', 'adjoint_first_block_only'),
        dict(block=256, waves=4, trips=2, col_blocks=2, last_live=44, strips=2, RS=1), uv_Sx=(0, 2), cls_Sx=(0, 2), pol=((7, 300, 2, 0, 5), 3, 4))
    add('w513', (3, 513, 1, 0, 4), 'eht_fwd_kernel: three column trips, one live lane in the last; eht_adjoint_kernel: three column blocks, one strip '
        'with H = 3 < EHT_ADJ_ROWS', fwd + ('first_trip_only', 'adjoint_first_block_only'), dict(block=256, trips=3, col_blocks=3, last_live=1, strips=1),
        cls_Sx=(0,), pol=((3, 513, 1, 0, 4), 3))
    add('h97_s20', (97, 7, 1, 0, 20), 'eht_row_splits: kblocks 24 -> rs 11 (below most = 13), rows_per 9, RS 11 with a last split of 7 rows; '
        'eht_columns: r1 clipped to H; eht_combine over 11 partial sums', ('last_split_dropped',),
        dict(nvis=190, kblocks=24, RS=11, rows_per=9, last_rows=7, block=64))
    add('h520', (520, 3, 1, 1, 4), 'eht_row_splits: rs 256 -> most 65 -> EHT_MAX_SPLITS 64 -> rows_per 9 -> RS 58, a last split of 7 rows; 130 '
        'adjoint strips', ('last_split_dropped',), dict(kblocks=1, RS=58, rows_per=9, last_rows=7, strips=130), cls_Sx=(0,), pol=((520, 3, 1, 1, 4), 3))
    add('s24', (8, 8, 1, 0, 24), 'eht_loss_kernel, cls_loss_kernel, pol_loss_kernel: nvis 276, ncp 2024, nca 21252 -- the second trip of `k += 256`, '
        'and of the triangle and quadrangle loops', ('first_256_baselines',), dict(nvis=276, ncp=2024, nca=21252, kblocks=35, RS=1),
        cls_Sx=(0,), pol=((8, 8, 1, 0, 24), 3, 4))
    add('n260', (16, 16, 260, 8, 4), 'eht_loss_sum_kernel, eht_terms_sum_kernel<3> (260 planes), eht_terms_sum_kernel<2> (257 frames): the second trip of '
        '`i += 256`; eht_twiddle_kernel: a grid over 260 frames', ('first_256_planes',), dict(N=260, RS=2), cls_Sx=(0,), pol=((8, 8, 257, 30, 4), 3))
    add('turns', (12, 20, 1, 1, 5), 'eht_twiddle: `t -= rint(t)` with thousands of whole turns in u x (field of view 10000 x FOV)', ('float32_phase',),
        dict(block=64, RS=2), uv=('vis', 'amp'), fov=10000.0 * E.FOV)
    add('one', (1, 1, 1, 0, 3), 'one pixel, one triangle: the twiddles at the centre pixel are (1, 0), every visibility is the pixel value', (),
        dict(nvis=3, ncp=1, nca=0, kblocks=1, RS=1, rows_per=1, block=64, trips=1, strips=1, last_live=1))
    return C


CASES = _cases()
# Worst error against float64 measured on an MI355X (tests/test_gpu_eht_edges.py prints every figure; DESIGN 4.10, 'edge shapes'):
# (case, Sx) -> (loss: the worst term or total, relative; dimages: relative to the largest element), per library.  A record, not a
# bound: every figure is held to its family's existing bound, none of which had to be derived anew.  libbhnerf_eht.so: the worst of
# 'vis', 'amp', 'cphase'; its visibilities are within 1.7e-7 (h520).  The host programs give 4e-6 at most on the same cases.
MEASURED = {
    'uv': {('w65', 0): (7.7e-7, 8.5e-7), ('w130', 0): (4.1e-7, 1.3e-6), ('w256', 0): (9.4e-8, 4.4e-7), ('w300', 0): (1.1e-6, 1.5e-6),
           ('w300', 2): (1.9e-7, 6.9e-7), ('w513', 0): (3.6e-7, 6.9e-7), ('h97_s20', 0): (4.9e-8, 6.5e-7), ('h520', 0): (1.3e-7, 9.2e-7),
           ('s24', 0): (9.9e-8, 4.4e-7), ('n260', 0): (3.0e-7, 3.7e-7), ('turns', 0): (2.3e-7, 3.0e-7), ('one', 0): (0.0, 0.0)},
    'cls': {('w130', 0): (5.1e-7, 7.4e-7), ('w300', 0): (1.1e-6, 6.4e-7), ('w300', 2): (1.9e-7, 1.2e-6), ('w513', 0): (3.6e-7, 3.7e-7),
            ('h520', 0): (8.7e-7, 4.7e-7), ('s24', 0): (9.9e-8, 2.8e-7), ('n260', 0): (3.0e-7, 1.8e-7)},
    'pol': {('w130', 3): (3.3e-8, 1.9e-7), ('w300', 3): (1.4e-7, 1.8e-7), ('w300', 4): (1.0e-7, 1.3e-7), ('w513', 3): (8.8e-8, 2.1e-7),
            ('h520', 3): (6.8e-7, 1.3e-6), ('s24', 3): (8.0e-8, 2.0e-7), ('s24', 4): (7.1e-8, 3.0e-7), ('n260', 3): (5.0e-8, 2.5e-7)},
}
BY_NAME = {c.name: c for c in CASES}
UV_PARAMS = [(c.name, Sx) for c in CASES for Sx in c.uv_Sx]
CLS_PARAMS = [(c.name, Sx) for c in CASES for Sx in c.cls_Sx]
POL_PARAMS = [(c.name, Sx) for c in CASES if c.pol for Sx in c.pol[1:]]
CONTRACT = ('w300', 'w513', 'h520')                       # the caller-owned-buffer contract, in each library


# ---- the inputs and clean references of a case, in each family's own form
def uv(name, Sx=0):
    c = BY_NAME[name]
    return E.case(name, Sx, spec=c.spec, fov=c.fov)


def cls(name, Sx=0):
    return K.case(name, Sx, spec=BY_NAME[name].spec)


def pol(name, Sx):
    return P.case(name, Sx, spec=BY_NAME[name].pol[0])


def admitted(name):
    """Asserts the admission conditions of every form of the case; returns the ratios."""
    c, out = BY_NAME[name], {}
    closures = 'cphase' in c.uv
    for Sx in c.uv_Sx:
        out['uv', Sx] = uv(name, Sx)['min_amp']
    for Sx in c.cls_Sx:
        assert closures, name
        out['cls', Sx] = cls(name, Sx)['min_amp']
    for Sx in (c.pol[1:] if c.pol else ()):
        out['pol', Sx] = pol(name, Sx)['min_amp']
    assert all(v >= E.MIN_AMP for k, v in out.items() if closures or k[0] == 'pol'), (name, out)
    if name == 's24':
        assert len(uv(name)['pairs']) == 276 and len(cls(name)['tri']) == 2024 and len(cls(name)['quad']) == 21252
    if name == 'turns':                                     # thousands of whole turns, and a baseline the field resolves out
        d = uv(name)
        turns = np.abs(d['uv']).max(axis=(0, 1)) * np.array([(c.W - 1) / 2.0 / c.W, (c.H - 1) / 2.0 / c.H]) * c.fov
        assert turns.max() >= 1000.0 and d['min_amp'] < E.MIN_AMP, (turns, d['min_amp'])
        out['turns'] = float(turns.max())
    return out


# ---- bounds: each family's own, unchanged
def uv_bound(dtype, what):
    return E.F32_TOL


def cls_bound(terms, what):
    """what: 'loss' or 'dimages' (test_gpu_closure._bound)."""
    return CLS_LOGCAMP_BOUND[what] if 'logcamp' in terms else E.F32_TOL


pol_bound = P.bound


# ---- the mutants
def dense_f32_phase(uvw, fov, H, W):
    """E.dense128 with the slip 'float32_phase': pixel coordinate, baseline coordinate and their product u x in turns are float32;
    the reduction to a turn and the sine and cosine are exact."""
    f = np.float32
    x = ((np.arange(W) - (W - 1) / 2.0) * (fov / W)).astype(f)
    y = ((np.arange(H) - (H - 1) / 2.0) * (fov / H)).astype(f)
    tu = (uvw[..., 0:1].astype(f) * x).astype(np.float64)                       # (B, nvis, W), rounded to float32
    tv = (uvw[..., 1:2].astype(f) * y).astype(np.float64)
    eu, ev = np.exp(-2j * np.pi * (tu - np.rint(tu))), np.exp(-2j * np.pi * (tv - np.rint(tv)))
    return (ev[..., :, None] * eu[..., None, :]).reshape(uvw.shape[:-1] + (H * W,))


def _operator(d, mutant, fov=E.FOV):
    """The dense float64 operator of a case dict with a forward slip built in."""
    H, W, A = d['H'], d['W'], d['A128']
    p = plan(1, A.shape[1], H, W)
    keep = np.ones((H, W), dtype=bool)
    x = np.arange(W)
    if mutant == 'first_wave_only':
        keep[:, (x % p['block']) >= WAVE] = False
    elif mutant == 'first_trip_only':
        keep[:, x >= LANES] = False
    elif mutant == 'last_split_dropped':
        keep[(p['RS'] - 1) * p['rows_per']:] = False
    elif mutant == 'float32_phase':
        return dense_f32_phase(d['uv'], fov, H, W)
    else:
        return A
    assert not keep.all(), (mutant, H, W)                   # the slip has something to drop
    return A * keep.reshape(-1)


def _adjoint_slip(grad, mutant):
    if mutant == 'adjoint_first_block_only':
        grad = grad.copy()
        assert grad.shape[-1] > LANES
        grad[..., LANES:] = 0.0
    return grad


def uv_reference(name, Sx, dtype, mutant=None):
    """(loss, dimages, visibilities or None) in float64 at scale 1: the reference of eht_uv_cases with `mutant` built in."""
    d = uv(name, Sx)
    if mutant is None:
        return d['ref'][dtype]
    assert mutant in MUTANTS
    A, (tg, sg), tri, sign = _operator(d, mutant, BY_NAME[name].fov), d['data'][dtype], d['tri'], d['sign']
    if mutant == 'first_256_baselines':
        assert tg.shape[-1] > LANES
        if dtype == 'cphase':
            loss, grad, _ = E.table_loss(d['images'], A, tg[..., :LANES], sg[..., :LANES], 1.0, dtype, tri[:LANES], sign[:LANES])
        else:
            loss, grad, _ = E.table_loss(d['images'], A[:, :LANES], tg[..., :LANES], sg[..., :LANES], 1.0, dtype)
        return loss, grad, None
    loss, grad, vis = E.table_loss(d['images'], A, tg, sg, 1.0, dtype, tri, sign)
    if mutant == 'first_256_planes':
        assert Sx == 0 and d['B'] > LANES
        loss = E.table_loss(d['images'][:LANES], A[:LANES], tg[:LANES], sg[:LANES], 1.0, dtype, tri, sign)[0]
    return loss, _adjoint_slip(grad, mutant), vis


def cls_reference(name, Sx, mutant=None):
    """(total, dimages, {term: value}, visibilities or None) of CLS_DTYPE at closure_cases.WEIGHTS and CLS_SCALE."""
    d = cls(name, Sx)
    if mutant is None:
        return K.reference(d, CLS_DTYPE, K.WEIGHTS, CLS_SCALE)
    assert mutant in MUTANTS
    A, terms = _operator(d, mutant), CLS_DTYPE.split('+')
    run = lambda A, data, terms, cut=None, frames=slice(None): K.closure_loss(
        d['images'][frames], A[frames], {t: (v[0][frames], v[1][frames]) for t, v in data.items()}, terms, K.WEIGHTS, CLS_SCALE,
        d['tri'][:cut], d['sign'][:cut], d['quad'][:cut])
    if mutant == 'first_256_baselines':
        assert min(len(d['pairs']), len(d['tri']), len(d['quad'])) > LANES
        data = {t: (v[0][..., :LANES], v[1][..., :LANES]) for t, v in d['data'].items()}
        ta, ga, pa, _ = run(A[:, :LANES], data, ['amp'])
        tc, gc, pc, _ = run(A, data, ['cphase', 'logcamp'], LANES)
        return ta + tc, ga + gc, dict(pa, **pc), None
    total, grad, parts, vis = run(A, d['data'], terms)
    if mutant == 'first_256_planes':
        assert Sx == 0 and d['B'] > LANES
        total, _, parts, _ = run(A, d['data'], terms, None, slice(0, LANES))
    return total, _adjoint_slip(grad, mutant), parts, vis


def pol_reference(name, Sx, mutant=None):
    """(total, dimages, {term: value}, visibilities or None) of POL_DTYPE at pol_cases.WEIGHTS and pol_cases.SCALE."""
    d = pol(name, Sx)
    if mutant is None:
        return P.reference(d, POL_DTYPE, P.WEIGHTS, P.SCALE)
    assert mutant in MUTANTS
    A, terms = _operator(d, mutant), POL_DTYPE.split('+')
    w = dict({t: 1.0 for t in P.TERMS}, **P.WEIGHTS)
    if mutant == 'first_256_baselines':
        assert len(d['pairs']) > LANES
        data = {t: (v[0][:, :LANES], v[1][:, :LANES]) for t, v in d['data'].items()}
        return P.pol_loss(d['images'], A[:, :LANES], data, terms, w, P.SCALE)[:3] + (None,)
    total, grad, parts, vis = P.pol_loss(d['images'], A, d['data'], terms, w, P.SCALE)
    if mutant == 'first_256_planes':
        assert d['B'] > LANES                               # frames: eht_terms_sum_kernel<2> strides over them
        total, _, parts, _ = P.pol_loss(d['images'][:LANES], A[:LANES], {t: (v[0][:LANES], v[1][:LANES]) for t, v in d['data'].items()}, terms, w, P.SCALE)
    return total, _adjoint_slip(grad, mutant), parts, vis


def rel_loss(got, want):
    """|got - want| / |want|; a reference of exactly 0 ('one': the data are the pixel itself) admits exactly 0 only."""
    return abs(got - want) / abs(want) if want != 0 else (0.0 if got == 0 else np.inf)


def rel_max(got, want):
    """eht_uv_cases.rel_max; an all-zero reference admits all zeros only."""
    return E.rel_max(got, want) if np.any(want) else (0.0 if not np.any(got) else np.inf)


def differences(clean, bad):
    """How far a mutant's (loss, dimages, ..., visibilities) is from the clean reference's: {'loss' relative, 'dimages' and 'vis'
    relative to the largest element of the clean one} -- the denominators of every family's bound."""
    out = {'loss': abs(bad[0] - clean[0]) / abs(clean[0]), 'dimages': E.rel_max(bad[1], clean[1])}
    if bad[-1] is not None:
        out['vis'] = E.rel_max(bad[-1], clean[-1])
    return out
