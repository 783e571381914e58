"""Rounding-faithful CPU emulator of the bf16 mode (float64 arithmetic, bf16 rounding where the kernels round) -- TEST ONLY.

``oracle_torch`` is the exact (float64) model: against it the bf16 kernels can only be held to the bf16 QUANTISATION noise
(a few per cent of the gradient on the small fixtures).  This module evaluates the same hot path in float64 but rounds every
value the kernels turn into an MFMA operand to bf16 at the kernels' own rounding point, and writes the backward out by hand
(the rounding is not differentiable, so autograd cannot produce it).  What is left between a kernel and this emulator is its
f32 accumulation order and the rare bf16 rounding that order flips: the tests hold the bf16 paths to that.

Forward (every path, ``fused_common.h``, ``general_mlp.hip``):
  * warp, posenc, masks, sigmoid and the ray sum in float64 from the f32-rounded inputs (the kernels: f32, ``t_M`` in f64);
  * packed weights bf16 (``fused_fwd.hip: pack_weights_kernel``, ``general_mlp.hip: gen_pack16_kernel``), biases f32: they are
    the initial accumulator (``fused_common.h: bias_acc``);
  * encoded inputs bf16 (``point_prologue``: ``Pol::set``; general path ``enc_put``);
  * hidden activations bf16: fused kernels round FIRST, then clamp the bf16 halves as signed integers, -0 -> +0
    (``fused_common.h: relu_pair``); the general path clamps the f32 accumulator, then rounds (``gen_mlp16_kernel``: ``on ? acc :
    0``).  relu' = (the bf16 activation > 0) in both: the recorded relu bits.
  * the output layer is an MFMA on bf16 ``h_D`` (and bf16 encoded inputs under a skip into it) with its f32 bias.

Backward: ``dout = dE e (1 - e)`` (f32 in the kernels, ``fused_bwd.hip`` chain_kernel "e ; dE, dout"); the delta chain
``gA_{l-1} = relu'_{l-1} (.) bf16(K_l gA_l)`` on bf16 transposed weight images; ``dW_l = x_l^T gA_l`` and ``db_l = sum gA_l`` on
the bf16 operands (``v_dot2`` / ``sum8``, or the slot-31 "1" column of the encoded-input tile under ``ga0_chain`` / fused128 --
the same sum).  The paths differ in the top of the chain (``RECIPES``).

Matrix products accumulate in float64 (torch CPU, multi-threaded).  ``rounding=False`` turns every bf16 rounding off: the
result is then the float64 model of ``oracle_torch`` (``tests/test_oracle_bf16_cpu.py`` checks it to 1e-12 for every recipe --
which is what shows the W_out fold and the fused 4x128 output-row identity are algebraically right).
"""
import numpy as np
import torch

from . import oracle_torch as ot

# --------------------------------------------------------------------------------------------------------------------------
# Per-path recipes.  Keys:
#   fold        gA_{D-1} is never formed: the chain's B operand is relu' (.) bf16(dout) against a transposed image of layer D-1
#               whose columns are pre-scaled by W_out, bf16(f32(K_{D-1}[j, k] W_out[k])); dW_{D-1} and db_{D-1} are the sums on
#               relu' (.) bf16(dout), multiplied by W_out[k] in f32 at the flush.  Else gA_{D-1} = bf16(f32(relu' W_out[k] dout)).
#   out_row     how dW_out (the hidden part) is formed: 'hD' = sum_p bf16(dout_p) h_D[p] on the recorded bf16 h_D;
#               'KG' = sum_k K[k][o] G[k][o] + b[o] g[o] from the un-folded gradient of layer D-1 = sum_p bf16(dout_p) relu(a_{D-1})
#               with the UNROUNDED pre-activation (no h_D on the tape).
#   out_bias    'dout' = sum of the f32 dout; 'bf16' = sum of bf16(dout) (the A tile / B column the output job multiplies).
#   relu        'round_clamp' (fused kernels) or 'clamp_round' (general path).
# --------------------------------------------------------------------------------------------------------------------------
RECIPES = {
    # (a) generic tape backward without the fold: bf16 depth 2 (bhn_folds_wout, common.h).
    #     gA_{D-1}: fused_bwd.hip chain_kernel, "g[r] = relu' ? wv4[e4] * dout : 0" then Pol::set (bf16), f32 W_out (wout_lds);
    #     dW_out / db_out: the output dW job's A operand is the dout tile, Pol::set(d0, 0, d) -> bf16; bias by Pol::sum8 of it.
    'generic': dict(fold=False, out_row='hD', out_bias='bf16', relu='round_clamp'),
    # (b) W_out fold / drop_ga, bf16 depth >= 3 (common.h bhn_folds_wout; fused_fwd.hip pack_weights_kernel "v *= W_out[o]").
    #     chain B operand: fused_bwd.hip chain_kernel "relu' (.) bf16(dout)" (d2 = {(__bf16)dout, ...});
    #     dW_{D-1}: dw_body2<LAST> "ga[i] = dpk & on", flush_tile "v[e] *= w4[e]", bias flush_column0(bsum * wout_r);
    #     output row: "dW_out[f] += dout_p h_depth[p][f], bf16 operands (v_dot2c)"; output bias: "bout += da[0] + ..." (f32 dout).
    'fold': dict(fold=True, out_row='hD', out_bias='dout', relu='round_clamp'),
    # (c) ga0_chain (width 256, depth >= 3): the fold of (b); dW_0 = gA_0^T enc is accumulated by the delta chain itself with the
    #     bias in the slot-31 "1" column of the encoded-input tile (fused_bwd.hip chain_kernel GA0C) -- the same sum of bf16 gA_0.
    'ga0_chain': dict(fold=True, out_row='hD', out_bias='dout', relu='round_clamp'),
    # (d) fused 4x128 (fused_bwd128.hip): front "gA_{depth-1} (without W_out) = relu' (.) bf16(dout)", the fold of (b) in the
    #     reduce ("if (fold) val *= wout[o]"); reduce128_kernel forms dW_out[o] = sum_k K[k][o] G[k][o] + b[o] g[o] from bf16 K and
    #     f32 b (no h_D on the tape: TapeLayout::drop_hd); output bias = the four waves' sums of f32 dout (tile 64, "bout").
    'fused128': dict(fold=True, out_row='KG', out_bias='dout', relu='round_clamp'),
    # (e) general path, bf16 mode (general_mlp.hip): hidden "f = (__bf16)(on ? acc : 0)" with on = acc > 0 (clamp, then round);
    #     gA_{D-1} "(__bf16)(relu' ? kf[r] * dv : 0)" with the f32 W_out; chain "(__bf16)(mask ? acc : 0)" on the unscaled bf16
    #     transposed image; gen_dw16_kernel: output job B = "(__bf16)dv" (bf16 dout), bias job A = ones (sum of the bf16 B operand).
    'general': dict(fold=False, out_row='hD', out_bias='bf16', relu='clamp_round'),
}

# Deliberately wrong variants of the faithful emulator (tests/test_oracle_bf16_cpu.py: the GPU bounds must be able to see them)
MUTANTS = ('drop_group', 'bias_scale', 'act_truncate', 'dout_unrounded')


def flat(grads):
    """[dK_0..dK_D, db_0..db_D] -> one float64 vector in flax tree order (kernel_0, bias_0, kernel_1, ...)."""
    n = len(grads) // 2
    return torch.cat([torch.cat([grads[i].reshape(-1), grads[n + i].reshape(-1)]) for i in range(n)]).numpy()


def recipe_for(flags):
    """The recipe of the path an engine's bhn_tape_info flags name (engine.tape_info()['flags'])."""
    if flags.get('general'):
        return 'general'
    if flags.get('fused128'):
        return 'fused128'
    if flags.get('ga0_chain'):
        return 'ga0_chain'
    if flags.get('drop_ga'):
        return 'fold'
    return 'generic'


# --------------------------------------------------------------------------------------------------------------------------
# Rounding
# --------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x32):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite inputs; NaN stays NaN)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bits_to_f32(b16):
    return (np.asarray(b16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x, mode='rne'):
    """float64 tensor/array -> the bf16 value of its f32 rounding (the kernels hold the value in f32 and convert), as float64.
    mode 'rne' (v_cvt_pk_bf16_f32), 'trunc' (drop the low 16 bits: a mutant), None (no rounding)."""
    if mode is None:
        return x
    is_t = torch.is_tensor(x)
    a = x.detach().cpu().numpy() if is_t else np.asarray(x)
    f = a.astype(np.float32)
    if mode == 'rne':
        r = bits_to_f32(bf16_bits(f))
    elif mode == 'trunc':
        r = (np.ascontiguousarray(f).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    else:
        raise ValueError(mode)
    r = r.astype(np.float64)
    return torch.from_numpy(r).to(x.dtype) if is_t else r


def round_f32(x, on=True):
    if not on:
        return x
    return x.to(torch.float32).to(torch.float64)


def relu_bf16(a, convention='round_clamp', mode='rne'):
    """The kernels' activation: 'round_clamp' = bf16 first, then the halves clamped as signed integers (-0 -> +0, fused_common.h
    relu_pair); 'clamp_round' = f32 max(a, 0), then bf16 (general_mlp.hip).  Returns (h, relu') with relu' = h > 0."""
    if convention == 'round_clamp':
        r = round_bf16(a, mode)
        h = torch.where(r > 0, r, torch.zeros_like(r))           # sign bit set (negative or -0) -> +0
    elif convention == 'clamp_round':
        h = round_bf16(torch.clamp(a, min=0.0), mode)
        h = torch.where(h > 0, h, torch.zeros_like(h))
    else:
        raise ValueError(convention)
    return h, h > 0


# --------------------------------------------------------------------------------------------------------------------------
# The emulator
# --------------------------------------------------------------------------------------------------------------------------
class Bf16Trainer:
    """Calling shapes of oracle_torch.CpuTrainer (kernels / biases as float64 tensors in flax tree order, `geom` / `hp` dicts, the
    `(b, *sp, G)` frame layout, 'full' / 'lc', Stokes J):  loss_and_grad(...) -> (loss, images, [dK_0..dK_D, db_0..db_D]).
    `recipe` names an entry of RECIPES; rounding=False: every bf16 rounding off (== the float64 model); `mutant` one of MUTANTS."""

    def __init__(self, kernels, biases, geom, hp, recipe='generic', rounding=True, mutant=None, accum32=False):
        if recipe not in RECIPES:
            raise ValueError('unknown recipe %r' % (recipe,))
        if mutant is not None and mutant not in MUTANTS:
            raise ValueError('unknown mutant %r' % (mutant,))
        self.k = [torch.as_tensor(k, dtype=torch.float64).detach() for k in kernels]
        self.b = [torch.as_tensor(b, dtype=torch.float64).detach() for b in biases]
        self.geom, self.hp = geom, hp
        self.rc = RECIPES[recipe]
        self.recipe, self.rounding, self.mutant = recipe, rounding, mutant
        # accum32: every matrix product and point sum accumulated in float32 (operands exact in f32) instead of float64 -- the
        # emulator with the kernels' precision of accumulation (not their order): its distance from the float64-accumulating
        # emulator measures how much accumulation noise alone moves a problem (tests/test_oracle_bf16_cpu.py)
        self.accum32 = accum32
        self.depth = int(hp['net_depth'])
        self.do_skip = hp.get('do_skip', True)
        assert len(self.k) == self.depth + 1

    def _mm(self, a, b):
        if self.accum32:
            return (a.to(torch.float32) @ b.to(torch.float32)).to(torch.float64)
        return a @ b

    def _sum0(self, x):
        if self.accum32:
            return x.to(torch.float32).sum(0).to(torch.float64)
        return x.sum(0)

    # rounding helpers bound to this instance's switches
    def _r(self, x):
        return round_bf16(x, 'rne' if self.rounding else None)

    def _act(self, a):
        if not self.rounding:
            h = torch.clamp(a, min=0.0)
            return h, h > 0
        return relu_bf16(a, self.rc['relu'], 'trunc' if self.mutant == 'act_truncate' else 'rne')

    def _skip_in(self):
        """skip_in[l]: layer l takes concat[h_l, enc] (network.py:59-61; the output layer too for odd depths / depth 2)."""
        D = self.depth
        s = [False] * (D + 1)
        if self.do_skip:
            sl = D // 2
            for i in range(D):
                if i % sl == 0 and i > 0:
                    s[i + 1] = True
        return s

    def _forward(self, t_frames):
        """-> dict of the per-point forward state (points flattened over (b, *sp, G))."""
        G, hp = self.geom, self.hp
        warped = ot.warp(G['coords'], G['Omega'], t_frames, G['t_start_obs'], G['t_geos'], G['t_injection'], hp['GM_c3'])
        valid = torch.isfinite(warped)
        net_in = torch.where(valid, warped, torch.zeros_like(warped))
        enc = ot.posenc(net_in / hp['scale'], hp.get('posenc_deg', 3))
        shape = enc.shape[:-1]
        enc = enc.reshape(-1, enc.shape[-1])
        enc_b = self._r(enc)
        D, skip = self.depth, self._skip_in()
        Kb = [self._r(k) for k in self.k]
        xs, acts, masks = [], [], []
        x = enc_b
        for l in range(D + 1):
            xin = torch.cat([x, enc_b], dim=-1) if skip[l] else x
            a = self._mm(xin, Kb[l]) + self.b[l]
            if self.accum32:
                a = round_f32(a)                                # (the f32 accumulator starts at the f32 bias)
            xs.append(xin)
            acts.append(a)
            if l < D:
                x, m = self._act(a)
                masks.append(m)
        out = acts[D][:, 0].reshape(shape)
        e = torch.sigmoid(out - 10.0)
        c = G['coords']
        r_sq = (c ** 2).sum(0)
        keep = ~((r_sq < hp['rmin'] ** 2) | (r_sq > hp['rmax'] ** 2) | (c[2].abs() > hp['z_width']))
        live = keep & valid[..., 0]
        e = torch.where(live, e, torch.zeros_like(e))
        return dict(enc_b=enc_b, Kb=Kb, xs=xs, acts=acts, masks=masks, e=e, live=live, shape=shape, skip=skip)

    def relu_tie_points(self, t_frames, rel=64 * 2.0 ** -23):
        """conftest.relu_tie_count's criterion on THIS forward (bf16 operands): boolean (*sp, G) of the ray samples with a hidden
        pre-activation |a| <= rel (|x| @ |K| + |b|) in any frame -- where the kernels' f32 accumulation may decide relu' (and
        the bf16 activation) the other way."""
        st = self._forward(t_frames)
        near = torch.zeros(st['acts'][0].shape[0], dtype=torch.bool)
        live = st['live'].reshape(-1)
        for l in range(self.depth):
            x, a = st['xs'][l], st['acts'][l]
            mag = x.abs() @ st['Kb'][l].abs() + self.b[l].abs()
            near |= ((a.abs() <= rel * mag) & live[:, None]).any(dim=-1)
        return near.reshape(st['shape']).any(dim=0).numpy()

    def emission(self, t_frames):
        """predictor (network.py:219-233) -> emission (b, *sp)."""
        return self._forward(t_frames)['e']

    def forward(self, t_frames):
        """images (b, H, W) or (b, S, H, W) as oracle_torch.render."""
        return ot.render(self._forward(t_frames)['e'], self.geom.get('J'), self.geom['g'], self.geom['dtau'], self.geom['Sigma'])

    def loss_and_grad(self, t_frames, target, sigma, offset, scale, dtype):
        return self._loss_and_grad(self._forward(t_frames), target, sigma, offset, scale, dtype)

    def loss_and_grad_variants(self, t_frames, target, sigma, offset, scale, dtype, mutants=MUTANTS):
        """{None: the faithful result, mutant: its result} for `mutants`, each (loss, images, grads); the backward-only mutants
        share the faithful forward (one forward for all but act_truncate)."""
        assert self.mutant is None
        st = self._forward(t_frames)
        out = {None: self._loss_and_grad(st, target, sigma, offset, scale, dtype)}
        try:
            for m in mutants:
                self.mutant = m
                out[m] = self._loss_and_grad(self._forward(t_frames) if m == 'act_truncate' else st, target, sigma, offset, scale, dtype)
        finally:
            self.mutant = None
        return out

    def _loss_and_grad(self, st, target, sigma, offset, scale, dtype):
        G = self.geom
        e = st['e'].clone().requires_grad_(True)
        images = ot.render(e, G.get('J'), G['g'], G['dtau'], G['Sigma'])
        loss = ot.loss_image(images, target, sigma, offset, scale, dtype)
        dE, = torch.autograd.grad(loss, e)          # sum_s dimg w_s: the chi^2 and the ray sum carry no bf16 rounding
        e = st['e']
        dout = torch.where(e != 0, dE * e * (1.0 - e), torch.zeros_like(e)).reshape(-1)
        dout = round_f32(dout, self.rounding)      # (the kernels form dout in f32)
        grads_k, grads_b = self._backward(st, dout)
        return loss.detach(), images.detach(), grads_k + grads_b

    def grad_linear(self, t_frames, dimages):
        """Gradient of sum(images * dimages) (what bhn_render_bwd / bhn_render_bwd_tape take: the upstream gradient of the images,
        shaped like forward()'s images) -> [dK_0..dK_D, db_0..db_D]."""
        st = self._forward(t_frames)
        G = self.geom
        e = st['e'].clone().requires_grad_(True)
        images = ot.render(e, G.get('J'), G['g'], G['dtau'], G['Sigma'])
        dE, = torch.autograd.grad((images * dimages).sum(), e)
        return self.grad_emission(st, dE)

    def state(self, t_frames):
        """The forward state grad_emission takes; its 'e' is the emission (b, *sp).  The ray sum and the loss carry no bf16 rounding,
        so several upstream gradients (tests/stokes4_cases.py: one per mutant of the Stokes planes) can share one forward."""
        return self._forward(t_frames)

    def grad_emission(self, st, dE):
        """The backward from dE = d loss / d emission (b, *sp) on the forward `st` -> [dK_0..dK_D, db_0..db_D]: grad_linear's
        arithmetic from its dE on."""
        e = st['e']
        dout = torch.where(e != 0, dE * e * (1.0 - e), torch.zeros_like(e)).reshape(-1)
        grads_k, grads_b = self._backward(st, round_f32(dout, self.rounding))
        return grads_k + grads_b

    def _backward(self, st, dout):
        rc, D = self.rc, self.depth
        rnd = self.rounding
        Kb, xs, acts, masks, skip = st['Kb'], st['xs'], st['acts'], st['masks'], st['skip']
        nh = [k.shape[1] for k in self.k]                       # hidden width of each layer's output
        dob = dout if self.mutant == 'dout_unrounded' else self._r(dout)
        dK, db = [None] * (D + 1), [None] * (D + 1)
        # sum over points, with one 32-point group left out for the 'drop_group' mutant
        wsel = torch.ones_like(dout)
        if self.mutant == 'drop_group':
            live = torch.nonzero(dout != 0).reshape(-1)
            if len(live):
                g0 = int(live[len(live) // 2]) // 32 * 32
                wsel[g0:g0 + 32] = 0.0
        xT = lambda x: (x * wsel[:, None]).T
        wout = self.k[D][:nh[D - 1], 0]                      # f32 W_out (wout_lds / the f32 image)
        # ---- top of the chain ----
        m = masks[D - 1].to(torch.float64)
        if rc['fold']:
            gu = m * dob[:, None]                               # relu' (.) bf16(dout): the B operand, W_out not applied
            G_un = self._mm(xT(xs[D - 1]), gu)                  # the un-folded dW_{D-1} and db_{D-1} sums
            g_un = self._sum0(gu * wsel[:, None])
            dK[D - 1] = G_un * wout[None, :]
            db[D - 1] = g_un * wout
            Kf = self._r(round_f32(self.k[D - 1][:nh[D - 2], :] * wout[None, :], rnd))   # bf16(f32(K W_out)) (pack_weights_kernel)
            ga = gu
            Kchain = Kf
        else:
            ga = self._r(round_f32(m * wout[None, :] * dout[:, None], rnd))
            dK[D - 1] = self._mm(xT(xs[D - 1]), ga)
            db[D - 1] = self._sum0(ga * wsel[:, None])
            Kchain = Kb[D - 1][:nh[D - 2], :]
        # ---- output layer ----
        dK[D] = self._mm(xT(xs[D]), dob[:, None])
        if rc['out_row'] == 'KG':
            # dW_out[o] = sum_k K[k][o] G[k][o] + b[o] g[o] (bf16 K of the forward, f32 b, G / g un-folded): the row on h_D
            # without h_D -- in exact arithmetic sum_p bf16(dout_p) relu(a_{D-1}), the pre-activation NOT rounded
            assert rc['fold']
            dK[D][:nh[D - 1], 0] = (Kb[D - 1] * G_un).sum(0) + self.b[D - 1] * g_un
        db[D] = self._sum0(((dout if rc['out_bias'] == 'dout' else dob) * wsel)[:, None])
        if self.mutant == 'bias_scale':
            db[D] = db[D] * (1.0 + 2.0 ** -8)
        # ---- delta chain: gA_{l-1} = relu'_{l-1} (.) bf16(K_l[hidden rows] gA_l) ----
        for l in range(D - 1, 0, -1):
            pre = self._mm(ga, Kchain.T)
            ga = masks[l - 1].to(torch.float64) * self._r(pre)
            dK[l - 1] = self._mm(xT(xs[l - 1]), ga)
            db[l - 1] = self._sum0(ga * wsel[:, None])
            if l - 1 > 0:
                Kchain = Kb[l - 1][:nh[l - 2], :]
        return dK, db
