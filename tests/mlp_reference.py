"""The one place where the reference of an MLP case is made, cached and frozen, and where its tied ray samples are found.  CPU only
(no CUDA call, at import or later); no test here.  tests/test_mlp_harness_cpu.py holds it to its rules.

Which reference serves which family: linear_reference -- emission, images and the gradient of sum(images * dimg) of a
frame_chunk_cases.build_problem dict -- serves test_gpu_frame_chunks (its ['grad']), test_gpu_buffer_contract and
test_gpu_general_path; Reference, which keeps the emission and gives images and gradients for any Stokes weights and any
upstream gradient (the mutants and chi^2 cases need that), serves test_gpu_stokes4; test_gpu_bf16_faithful builds its emulator from a
tree and a geometry and takes only tie_points from here.  Both are the float64 oracle for `recipe` None and oracle_bf16's emulator of
`recipe` otherwise.  They stay two evaluation orders: linear_reference sums over the full ray grid, Reference over the in-domain
points only (the shell domains keep 6 to 30 % of the samples), and the float64 sums of the two differ in their last bits -- merging
them would move every recorded figure of one family."""
import numpy as np
import torch

from conftest import relu_tie_count
from mlp_problems import flat_grad, oracle_inputs, t64, without_samples
from oracle import oracle_bf16 as ob
from oracle import oracle_torch as ot

_CACHE = {}


def cached(family, case, what, recipe, drop, accum32, make):
    """make() of a case, made once and left unchanged: every numpy array of it (or of the dict it is) is read-only from here on.
    `drop` enters the key as dropped or not: a case is adjudicated with one mask."""
    key = (family, case, what, recipe, drop is not None, accum32)
    if key not in _CACHE:
        out = make()
        for v in (out.values() if isinstance(out, dict) else [out]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def dropped(prob, drop):
    """The problem without the ray samples `drop` (H, W, G) bool: Doppler weight 0 on both sides (the ReLU-tie adjudication);
    `drop` None: the problem itself."""
    return prob if drop is None else dict(prob, g=without_samples(prob['g'], drop))


def tie_points(g, em, tf, do_skip=True):
    """(H, W, G) bool: the ray samples that reach the image (Doppler weight != 0) and have a ReLU tie on the reference's own forward --
    `em` None: conftest.relu_tie_count's on the float64 model (which walks the skip network: without the skips, its criterion on the
    emulator with every rounding off); else em.relu_tie_points(tf), the same criterion on the bf16 forward."""
    if em is not None:
        ties = em.relu_tie_points(tf)
    elif do_skip:
        ties = relu_tie_count(g, return_points=True)[1]
    else:
        ks, bs, geom, hp = oracle_inputs(g)
        ties = ob.Bf16Trainer(ks, bs, geom, dict(hp, do_skip=False), rounding=False).relu_tie_points(tf)
    return ties & (np.broadcast_to(g['g'], ties.shape) != 0)


# ---- over the full ray grid: frame chunks, buffer contract, general path
def _linear(prob, recipe, drop, accum32, want_ties):
    prob = dropped(prob, drop)
    g, S = prob['g'], prob['S']
    ks, bs, geom, hp = oracle_inputs(g)
    do_skip = prob.get('do_skip', True)
    hp = hp if do_skip else dict(hp, do_skip=False)
    tf = t64(g['t_frames'])
    em = None if recipe is None else ob.Bf16Trainer(ks, bs, geom, hp, recipe, accum32=accum32)
    if want_ties:
        return tie_points(g, em, tf, do_skip)
    d_em = prob['dimg'].reshape((prob['B'], max(S, 1)) + prob['spatial'])
    d_em = d_em if S else d_em[:, 0]
    if em is None:
        e = ot.predictor(ks, bs, tf, geom['coords'], geom['Omega'], geom['t_start_obs'], geom['t_geos'], geom['t_injection'], hp['GM_c3'],
                         hp['scale'], hp['rmin'], hp['rmax'], hp['z_width'], posenc_deg=hp['posenc_deg'], net_depth=hp['net_depth'], do_skip=do_skip)
        grads = ot.grad_linear(ks, bs, geom, hp, tf, d_em)
    else:
        e = em.emission(tf)
        grads = em.grad_linear(tf, d_em)
    img = ot.render(e, geom['J'], geom['g'], geom['dtau'], geom['Sigma'])
    return dict(emission=e.detach().numpy().reshape(prob['B'], -1), images=img.detach().numpy().reshape(prob['B'], max(S, 1), -1), grad=ob.flat(grads))


def linear_reference(family, case, prob, recipe=None, drop=None, accum32=False, want_ties=False):
    """dict(emission (B, H*W*G), images (B, Sx, R), grad: the flat gradient of sum(images * dimg) in flax tree order), float64 arrays,
    of a frame_chunk_cases.build_problem dict (which may hold do_skip = False); accum32: the emulator accumulating in float32;
    want_ties: instead the tie_points of that reference."""
    return cached(family, case, 'ties' if want_ties else 'linear', recipe, drop, accum32, lambda: _linear(prob, recipe, drop, accum32, want_ties))


# ---- over the in-domain points: four Stokes planes
class Reference:
    """One forward of the float64 oracle (recipe None) or of the bf16 emulator of `recipe` on a problem's g: the emission, from which
    images(J) and grad(dimages, J) follow for any Stokes weights J (S, H, W, G) -- the render and the loss carry no bf16 rounding.
    Only the samples inside the recovery domain are evaluated, as points of their own (sp = (N,)): the others have emission 0
    whatever the parameters are (oracle_torch.predictor's mask)."""

    def __init__(self, g, recipe=None):
        ks, bs, geom, hp = oracle_inputs(g)
        self.tf = t64(g['t_frames'])
        self.J = geom['J']
        self.recipe = recipe
        c = geom['coords']
        self.shape = tuple(c.shape[1:])                                  # (H, W, G)
        r_sq = (c ** 2).sum(0)
        keep = ~((r_sq < hp['rmin'] ** 2) | (r_sq > hp['rmax'] ** 2) | (c[2].abs() > hp['z_width']))
        self.idx = torch.nonzero(keep.reshape(-1)).reshape(-1)
        self.ray = torch.div(self.idx, self.shape[-1], rounding_mode='floor')
        self.R = self.shape[0] * self.shape[1]
        take = lambda v: v.reshape(-1)[self.idx]
        self.w = take(geom['g'] ** 2 * geom['dtau'] * geom['Sigma'])
        pts = dict(coords=torch.stack([take(c[i]) for i in range(3)]), Omega=take(geom['Omega']), t_geos=take(geom['t_geos']))
        if recipe is None:
            self.params = [p.clone().requires_grad_(True) for p in ks + bs]
            n = len(ks)
            self.e = ot.predictor(self.params[:n], self.params[n:], self.tf, pts['coords'], pts['Omega'], geom['t_start_obs'], pts['t_geos'],
                                  geom['t_injection'], hp['GM_c3'], hp['scale'], hp['rmin'], hp['rmax'], hp['z_width'], hp['posenc_deg'],
                                  hp['net_depth'])
        else:
            self.em = ob.Bf16Trainer(ks, bs, dict(pts, t_start_obs=geom['t_start_obs'], t_injection=geom['t_injection']), hp, recipe)
            self.st = self.em.state(self.tf)
            self.e = self.st['e']
        assert tuple(self.e.shape) == (len(self.tf), len(self.idx))

    def _Jw(self, J):
        J = self.J if J is None else J
        return J.reshape(J.shape[0], -1)[:, self.idx] * self.w[None]

    def images(self, J=None):
        """(B, S, H, W), float64."""
        Jw = self._Jw(J)
        out = torch.zeros((len(self.tf), Jw.shape[0], self.R), dtype=torch.float64)
        out.index_add_(2, self.ray, self.e.detach()[:, None, :] * Jw[None])
        return out.reshape(out.shape[:2] + self.shape[:2])

    def grad(self, dimages, J=None):
        """The gradient of sum(images(J) * dimages), flat in flax tree order."""
        Jw = self._Jw(J)
        dE = (dimages.reshape(dimages.shape[0], Jw.shape[0], self.R)[:, :, self.ray] * Jw[None]).sum(dim=1)
        if self.recipe is None:
            return flat_grad(list(torch.autograd.grad(self.e, self.params, grad_outputs=dE, retain_graph=True)))
        return ob.flat(self.em.grad_emission(self.st, dE))

    def relu_tie_points(self, tf):
        """The emulator's tied points, back on the (H, W, G) grid."""
        ties = np.zeros(int(np.prod(self.shape)), dtype=bool)
        ties[self.idx.numpy()] = self.em.relu_tie_points(tf)
        return ties.reshape(self.shape)

    def relu_ties(self, g):
        """tie_points of this reference."""
        return tie_points(g, None if self.recipe is None else self, self.tf)


def point_reference(family, case, prob, recipe=None, drop=None):
    """The Reference of a case."""
    return cached(family, case, 'points', recipe, drop, False, lambda: Reference(dropped(prob, drop)['g'], recipe))
