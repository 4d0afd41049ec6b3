"""Host-only yardstick for ONE schedule step of the step engine (csrc/engine.cpp) from that step's own inputs: an fp64 reference built
from the oracle's blocks, an emulator of the engine's arithmetic with a bf16 rounding at every point where the engine stores bf16 (and
named mutants, each a plausible wiring error), and a per-element error budget.  tests/test_layer_ref_cpu.py proves the yardstick (the
clean emulator stays inside the budget, every mutant leaves it); tests/test_layers_gpu.py holds the engine to it, layer by layer, with
the engine's own taps as inputs (teacher forcing), so that depth does not accumulate.

Kinds: "t" / "v" a self layer (BertLayer / BertImageLayer), "c" a connection layer, "e" the two embeddings (the last backward segment:
reference_embed / emulate_embed / budget_embed), "h" the heads plus losses (segment 0: reference_heads / emulate_heads / budget_heads).

What the engine reads (engine.cpp, Run::gemm_args / ln_fwd / ln_bwd): the MATRIX of every Linear from the bf16 shadow (PB(l.w)); every
Linear BIAS and every LayerNorm weight / bias from the fp32 masters (g.bias = P(l.b), P(ln.g), P(ln.b)).  `weights_of` builds exactly
that dict from the two flat buffers.

Where the engine stores bf16 (self_fwd / proj_fwd / ffn_fwd / conn_fwd, the backward counterparts, gemm.hip's gemm_epilogue):
  forward   qkv;  the attention internals and ctx as attention_ref.emulate models them;  s = dropout(dense(ctx)) + residual (bf16, or
            fp32 under residual_fp32: then the residual is the fp32 copy of the producing LayerNorm's output);  the LayerNorm output a / y
            (bf16, plus the fp32 copy under residual_fp32);  u = the GELU pre-activation (rounded from the fp32 accumulator) and
            h = gelu(fp32 accumulator) (rounded once, not gelu of the rounded u).
  backward  dres (LayerNorm backward rows), dlin = dropout mask applied to the fp32 dres (stored only when p > 0), du = (dl W_down) gelu'(u)
            with the bf16 u, gc = du W_up + dres_a, dctx, dqkv (attention_ref.emulate), gx = dqkv W_qkv + dres_b.
  Parameter gradients are fp32 sums; the LayerNorm column sums (dgamma, dbeta, the producing Linear's bias gradient) add the kernel's
  fp32 row values, the QKV / FFN-up bias gradients add the bf16 dqkv / du.

The budget is a variance carried through the same graph in fp64, never a measurement: every bf16 storage point adds (2^-9 |value|)^2 --
the largest rounding error squared, i.e. three times the variance of a uniform rounding error -- every fp32 accumulation S32^2 times the
sum of its squared products, and every operation passes the incoming variances on through its SQUARED Jacobian (a Linear through W^2,
softmax / LayerNorm / GELU through the squares of their derivatives, a weight gradient through sum_rows of the squared products), which is
what independent rounding errors do.  budget = KSIGMA sqrt(variance).  A worst-case sum through |W| would be sqrt(K) = 28 ... 64 times
larger at these widths and lets a wrong dropout mask or a missing residual through.  Under residual_fp32 the tap of a layer input is
the bf16 copy of a tensor whose fp32 copy the engine adds as the residual: (2^-9 |x|)^2 enters s as one more term (x32=True).
Two places where errors are NOT independent are carried as such: what an attention inherits from dctx, q, k, v is spread over the rows of a
batch element, so a later sum over rows (weight and bias gradients of QKV and of the attention output projection) adds that part
coherently within a batch element (_Ar.wgrad); and the error of a row's delta_i reaches dq through sum_j P_ij k_j as ONE number
(_Attn.bwd) -- large where a key column has one sign over the keys, as the outlier channels of real hidden states give it; with kept row
statistics (beyond 112 keys or queries) delta_i = dctx_i . ctx_i carries everything the stored ctx carries.  The CPU test shows the clean
emulator at 1.19 of the quadrature form and 0.26 of this one on recorded inputs of a late layer (tests/golden/layer_v5_*.npz).
No absolute floors.  `ratio` adds one bf16 step at max(|got|, |ref|) for a bf16-stored output, as attention_ref.ratio does.
"""
import math

import torch

import attention_ref as AR
from oracle import crct_oracle as O

U9 = 2.0 ** -9            # largest relative error of one round-to-nearest bf16 storage
S32 = 2.0 ** -16          # fp32 accumulation slack, as attention_ref.S32
F32 = 2.0 ** -24
KSIGMA = 7.0              # chosen on the CPU (tests/test_layer_ref_cpu.py): the clean emulator's worst ratio stays below 0.9
EPS = O.LN_EPS
MUTANTS = ("ffn_residual_from_layer_input", "conn_ctx_swapped", "conn_wrong_keymask", "keymask_previous_row", "k_wgrad_from_v_slice",
           "dx_without_residual_path", "bias_grad_drops_last_row", "dropout_site_off_by_one", "stale_gradient_tile")
HEAD_MUTANTS = ("heads_cat_halves_swapped", "heads_reg_seed_without_batch_mean", "heads_pipe_row_overwrites_pooler_row")
EMBED_MUTANTS = ("embed_scatter_drops_last_row", "embed_loc_mask_ignored")

SELF = dict(q="attention.self.query", k="attention.self.key", v="attention.self.value", o="attention.output.dense",
            ln1="attention.output.LayerNorm", up="intermediate.dense", down="output.dense", ln2="output.LayerNorm")
CONN_V = dict(q="biattention.query1", k="biattention.key1", v="biattention.value1", o="biOutput.dense1", ln1="biOutput.LayerNorm1",
              up="v_intermediate.dense", down="v_output.dense", ln2="v_output.LayerNorm")
CONN_T = dict(q="biattention.query2", k="biattention.key2", v="biattention.value2", o="biOutput.dense2", ln1="biOutput.LayerNorm2",
              up="t_intermediate.dense", down="t_output.dense", ln2="t_output.LayerNorm")


def prefix_of(kind, idx):
    return "bert.encoder.%s.%d." % ({"t": "layer", "v": "v_layer", "c": "c_layer"}[kind], idx)


def weights_of(table, flat_params, flat_shadow, pre):
    """{name: fp64 tensor} of the parameters under prefix `pre` as the engine reads them: '.weight' of a Linear (2-D) from the bf16 shadow,
    everything else (biases, LayerNorm weight and bias) from the fp32 masters.  table: crct.layout entries (name, offset, numel, shape)."""
    sd = {}
    for e in table:
        if e.name.startswith(pre):
            src = flat_shadow if len(e.shape) == 2 else flat_params
            sd[e.name] = src[e.offset:e.offset + e.numel].detach().double().cpu().view(*e.shape)
    return sd


def ratio(got, ref, bud, stored_bf16):
    got, ref = got.double(), ref.double()
    den = bud + (AR.bf16_step(torch.maximum(got.abs(), ref.abs())) if stored_bf16 else 0.0)
    return (got - ref).abs() / den


def stored_bf16(name):
    """The step outputs and input gradients are bf16 buffers, the parameter gradients fp32."""
    return name.split("_")[0] in ("y", "gx")


def describe(what, name, got, ref, bud):
    """(worst ratio, failure message or None) of one output: the message names the step, the output, the count of offenders and the first
    offender's index, value, fp64 value, budget and ratio."""
    got, ref = got.double().cpu().reshape(ref.shape), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), "%s %s: non-finite output" % (what, name)
    r = ratio(got, ref, bud, stored_bf16(name))
    r = torch.where((got == ref), torch.zeros_like(r), r)          # 0 / 0: an exact zero that is zero
    bad = r > 1.0
    if not bool(bad.any()):
        return float(r.max()), None
    i = tuple(int(j) for j in bad.nonzero()[0])
    return float(r.max()), "%s %s: %d of %d elements beyond the budget, first at %s: got %r, fp64 %r, budget %r, ratio %.2f (worst %.2f)" % (
        what, name, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(bud[i]), float(r[i]), float(r.max()))


# ------------------------------------------------------------------------------------------- fp64 reference (oracle blocks + autograd)
class _MaskDrop:
    """Stands in for oracle._drop inside one block: call k multiplies by the k-th keep mask / (1 - p)."""

    def __init__(self, keeps, p):
        self.keeps, self.p, self.k = list(keeps), p, 0

    def __call__(self, x, prob, training):
        keep = self.keeps[self.k]
        self.k += 1
        assert tuple(keep.shape) == tuple(x.shape), (self.k, tuple(keep.shape), tuple(x.shape))
        return x * keep.to(x.dtype) / (1.0 - self.p)


def _add_mask(km):
    return (1.0 - torch.as_tensor(km).double())[:, None, None, :] * -10000.0


def _drop_list(kind, drops):
    if not drops:
        return None
    return [drops[k] for k in (("attn", "proj", "ffn") if kind != "c" else ("attn_t", "attn_v", "proj_v", "proj_t", "ffn_v", "ffn_t"))]


def reference(kind, sd, pre, cfg, x, dy, km, drops=None, p=0.0):
    """One schedule step in fp64 with torch autograd over the oracle's own block (O._self_layer / O._connection_layer).
    kind "t" / "v": x, dy [B, L, H], km [B, L] (1 = attended).  kind "c": x = (xv, xt), dy = (dyv, dyt), km = (km_v, km_t).
    sd: {full parameter name: value} as the engine reads them (weights_of).  drops: the engine's keep masks of the step's dropout sites
    ("attn", "proj", "ffn"; connection layer "attn_t" (text queries), "attn_v", "proj_v", "proj_t", "ffn_v", "ffn_t"), p their probability.
    Returns {"y" | "y_v", "y_t": outputs, "gx" | "gx_v", "gx_t": input gradients, parameter name without prefix: its gradient}."""
    w = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
    keeps = _drop_list(kind, drops) if p > 0 else None
    saved = O._drop
    if keeps is not None:
        O._drop = _MaskDrop(keeps, p)
    try:
        if kind == "c":
            xv, xt = (t.detach().double().clone().requires_grad_(True) for t in x)
            yv, yt = O._connection_layer(w, cfg, pre, xv, _add_mask(km[0]), xt, _add_mask(km[1]), keeps is not None)
            torch.autograd.backward([yv, yt], [dy[0].double(), dy[1].double()])
            out = dict(y_v=yv.detach(), y_t=yt.detach(), gx_v=xv.grad, gx_t=xt.grad)
        else:
            heads = cfg.num_attention_heads if kind == "t" else cfg.v_num_attention_heads
            xx = x.detach().double().clone().requires_grad_(True)
            y = O._self_layer(w, pre, xx, _add_mask(km), heads, p, p, keeps is not None)
            y.backward(dy.double())
            out = dict(y=y.detach(), gx=xx.grad)
    finally:
        O._drop = saved
    for k, v in w.items():
        if v.grad is not None:                      # (the connection layer's q_dense1 / q_dense2 are read by no block: no gradient)
            out[k[len(pre):]] = v.grad
    return out


# ------------------------------------------------------------------------------------------- the engine's arithmetic, two readings
class Q:
    """A quantity of the engine's graph: v its value (fp64 tensor) and, in the budget reading, e the variance bound of the engine's error."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v, self.e = v, e


def _rb(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


class _Ar:
    """bound=False: the emulator -- values carry the engine's roundings, matmuls and reductions run in `acc`.
    bound=True: the budget -- values are the fp64 ones, e carries the variance."""

    def __init__(self, bound, acc=torch.float64, mutate=None, independent_delta=False):
        self.bound, self.acc, self.mutate, self.independent_delta = bound, acc, mutate, independent_delta

    def exact(self, t, rel=0.0):
        v = t.detach().double()
        return Q(v, (rel * v) ** 2 if self.bound else None)

    def store(self, x):
        return Q(x.v, x.e + (U9 * x.v) ** 2) if self.bound else Q(_rb(x.v))

    def store32(self, x):
        return Q(x.v, x.e + (F32 * x.v) ** 2) if self.bound else Q(x.v.to(torch.float32).double())

    def mm(self, a, b):
        return a @ b if (self.bound or self.acc == torch.float64) else (a.to(self.acc) @ b.to(self.acc)).double()

    def lin(self, x, W, b=None):                  # x W^T + b, the fp32 accumulator
        v = self.mm(x.v, W.t())
        if b is not None:
            v = v + b
        W2 = (W * W).t()
        return Q(v, x.e @ W2 + S32 ** 2 * ((x.v ** 2) @ W2) if self.bound else None)

    def dgrad(self, dy, W):                       # dy W
        W2 = W * W
        return Q(self.mm(dy.v, W), dy.e @ W2 + S32 ** 2 * ((dy.v ** 2) @ W2) if self.bound else None)

    def wgrad(self, dy, x, dy_inh=None, x_inh=None):
        """dy^T x, stored fp32.  dy_inh / x_inh [B, L, width]: the part of dy's / x's variance whose errors are correlated over the rows
        of a batch element (what an attention spreads over its rows).  A sum over rows adds those coherently at worst:
        var(sum_j e_j) <= (sum_j sigma_j)^2 within a batch element, variances across batch elements."""
        v = self.mm(dy.v.t(), x.v)
        if not self.bound:
            return Q(v.to(torch.float32).double())
        d2, x2 = (dy.v ** 2).t(), x.v ** 2
        ed, ex = dy.e, x.e
        e = S32 ** 2 * (d2 @ x2)
        if dy_inh is not None:
            B = dy_inh.shape[0]
            ed = (ed - dy_inh.reshape(ed.shape)).clamp_min(0.0)
            e = e + ((torch.sqrt(dy_inh).transpose(-1, -2) @ x.v.abs().reshape(B, -1, x.v.shape[-1])) ** 2).sum(0)
        if x_inh is not None:
            B = x_inh.shape[0]
            ex = (ex - x_inh.reshape(ex.shape)).clamp_min(0.0)
            e = e + ((dy.v.abs().reshape(B, -1, dy.v.shape[-1]).transpose(-1, -2) @ torch.sqrt(x_inh)) ** 2).sum(0)
        # (the last term: both factors off at once, each by its whole budget -- |dg dx| <= (KSIGMA sigma_g) (KSIGMA sigma_x), in variance
        # units KSIGMA^2 e_g e_x.  Second order: visible only where a slope in doubt meets an activation at its kink, in the heads)
        return Q(v, e + ed.t() @ x2 + d2 @ ex + KSIGMA ** 2 * (ed.t() @ ex))

    def colsum(self, dy, rows=None, inh=None):
        v, e = (dy.v, dy.e) if rows is None else (dy.v[:rows], dy.e[:rows] if self.bound else None)
        if not self.bound:
            return Q(v.to(self.acc).sum(0).to(torch.float32).double())
        if inh is not None:
            e = (e - inh.reshape(e.shape)).clamp_min(0.0).sum(0) + (torch.sqrt(inh).sum(1) ** 2).sum(0)
        else:
            e = e.sum(0)
        return Q(v.sum(0), e + S32 ** 2 * (v ** 2).sum(0))

    def scale(self, x, m):                        # elementwise product with an exact tensor
        return Q(x.v * m, x.e * m * m if self.bound else None)

    def add(self, a, b):
        return Q(a.v + b.v, a.e + b.e if self.bound else None)


def _gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_d(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _gelu_dd(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) * (2.0 - x * x)


def _ln_fwd(ar, s, g, b):
    """y = g xhat + b in fp32 registers (not stored yet), xhat and rstd for the backward."""
    H = s.v.shape[-1]
    v = s.v if ar.bound else s.v.to(ar.acc)
    mu = v.mean(-1, keepdim=True)
    xc = v - mu
    r = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    xh = (xc * r).double()
    r = r.double()
    y = g * xh + b
    if not ar.bound:
        return Q(y), Q(xh), Q(r.to(torch.float32).double())
    e = s.e
    t2 = (xh * xh * e).sum(-1, keepdim=True) / H ** 2
    exh = r * r * (e + e.sum(-1, keepdim=True) / H ** 2 + xh * xh * t2) + (S32 * xh) ** 2
    return Q(y, g * g * exh + (S32 * y) ** 2), Q(xh, exh), Q(r, r ** 4 * t2 + (S32 * r) ** 2)


def _ln_bwd(ar, dy, xh, r, g):
    """(dres, dgamma, dbeta): the row pass in fp32 registers, the column sums over the rows."""
    H = dy.v.shape[-1]
    dxh = dy.v * g
    m1 = dxh.mean(-1, keepdim=True)
    m2 = (dxh * xh.v).mean(-1, keepdim=True)
    dres = r.v * (dxh - m1 - xh.v * m2)
    dg, db = (dy.v * xh.v), dy.v
    if not ar.bound:
        return Q(dres), Q(dg.to(ar.acc).sum(0).to(torch.float32).double()), Q(db.to(ar.acc).sum(0).to(torch.float32).double())
    ed = dy.e * g * g
    x2 = xh.v * xh.v
    e = r.v ** 2 * (ed + ed.sum(-1, keepdim=True) / H ** 2 + x2 * (x2 * ed).sum(-1, keepdim=True) / H ** 2)
    e = e + r.v ** 2 * (xh.e * m2 * m2 + x2 * (dxh * dxh * xh.e).sum(-1, keepdim=True) / H ** 2)
    e = e + (dres / r.v) ** 2 * r.e + (S32 * dres) ** 2
    edg = (dy.e * x2 + dy.v ** 2 * xh.e).sum(0) + S32 ** 2 * (dg * dg).sum(0)
    edb = dy.e.sum(0) + S32 ** 2 * (db * db).sum(0)
    return Q(dres, e), Q(dg.sum(0), edg), Q(db.sum(0), edb)


def _path(Tq, Tk):
    return "mfma" if Tq <= 112 and Tk <= 112 else "long"


def _hd(t, heads):
    B, T, H = t.shape
    return t.reshape(B, T, heads, H // heads).permute(0, 2, 1, 3)


def _rows(t):
    B, h, T, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, h * d)


class _Attn:
    """ctx = attention(q, k, v) and its backward.  Emulator: attention_ref.emulate (the kernels' documented arithmetic; the long-sequence
    kernels with kept row statistics, as the engine runs them).  Budget: the fp64 operation with the variances passed through."""

    def __init__(self, ar, q, k, v, km, heads, keep, p):
        self.ar, self.q, self.k, self.v, self.km, self.heads, self.keep, self.p = ar, q, k, v, torch.as_tensor(km).bool(), heads, keep, p
        self.d = q.v.shape[-1] // heads
        self.path = _path(q.v.shape[1], k.v.shape[1])

    def _emulate(self, dctx):
        bf = lambda t: t.to(torch.float32).to(torch.bfloat16)
        return AR.emulate(bf(self.q.v), bf(self.k.v), bf(self.v.v), self.km.to(torch.uint8), bf(dctx), self.heads, self.d,
                          keep=self.keep if self.p > 0 else None, p=self.p, path=self.path, kept=self.path == "long")

    def fwd(self):
        ar = self.ar
        if not ar.bound:
            return Q(self._emulate(torch.zeros_like(self.q.v))["ctx"])
        h, d = self.heads, self.d
        sc = 1.0 / math.sqrt(d)
        q, k, v = _hd(self.q.v, h), _hd(self.k.v, h), _hd(self.v.v, h)
        eq, ek, ev = _hd(self.q.e, h), _hd(self.k.e, h), _hd(self.v.e, h)
        s = q @ k.transpose(-1, -2) * sc + torch.where(self.km, 0.0, -10000.0)[:, None, None, :]
        es = sc * sc * (eq @ (k * k).transpose(-1, -2) + (q * q) @ ek.transpose(-1, -2))
        P = torch.softmax(s, -1)
        eP = P * P * (es + (P * P * es).sum(-1, keepdim=True)) + (S32 * P) ** 2
        ks = 1.0 / (1.0 - self.p) if self.p > 0 else 1.0
        kp = (self.keep.double() if self.p > 0 else torch.ones_like(P)) * ks
        Pd = P * kp
        ePd = eP * kp * kp + (U9 * Pd) ** 2                     # the probabilities are rounded to bf16 before P V
        ctx = Pd @ v
        ectx = ePd @ (v * v) + (Pd * Pd) @ ev
        self.c = (q, k, v, eq, ek, ev, P, eP, Pd, ePd, kp, sc, ctx, ectx)
        self.inh_ctx = _rows((ectx - ((U9 * Pd) ** 2) @ (v * v)).clamp_min(0.0))      # all but the rounding of the probabilities
        return ar.store(Q(_rows(ctx), _rows(ectx)))

    def bwd(self, dctx):
        ar = self.ar
        if not ar.bound:
            o = self._emulate(dctx.v)
            return Q(o["dq"]), Q(o["dk"]), Q(o["dv"])
        q, k, v, eq, ek, ev, P, eP, Pd, ePd, kp, sc, ctx, ectx = self.c
        g, eg = _hd(dctx.v, self.heads), _hd(dctx.e, self.heads)
        dP = (g @ v.transpose(-1, -2)) * kp
        edP = kp * kp * (eg @ (v * v).transpose(-1, -2) + (g * g) @ ev.transpose(-1, -2))
        delta = (P * dP).sum(-1, keepdim=True)
        if ar.independent_delta:
            # the tighter form the clean emulator leaves on real hidden states (test_delta_error_reaches_dq_as_one_number)
            edelta = (eP * dP * dP + P * P * edP).sum(-1, keepdim=True) + U9 ** 2 * (g * g * ctx * ctx).sum(-1, keepdim=True)
        elif self.path == "long":
            # kept row statistics (attention_long.hip with CrctAttnQuant.row_lse / ctx): delta_i = dctx_i . ctx_i from the forward's STORED
            # bf16 ctx, so delta carries everything ctx carries -- the rounding of the probabilities before P V and of ctx itself included,
            # which the sum over P dP of the other kernels does not see
            edelta = (eg * ctx * ctx + g * g * (ectx + (U9 * ctx) ** 2)).sum(-1, keepdim=True)
        else:
            edelta = (eP * dP * dP + P * P * edP).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        edS0 = eP * (dP - delta) ** 2 + P * P * edP + (U9 * dS) ** 2      # dS is rounded to bf16 before dS K / dS^T Q
        edS = edS0 + P * P * edelta
        dq = dS @ k * sc
        # the error of delta_i is ONE number for the whole row: it reaches dq_ic through sum_j P_ij k_jc, added coherently over the
        # keys (a key column with a common sign over j, as LayerNorm'd activations have, makes that sum large), not in quadrature
        if ar.independent_delta:
            edq = sc * sc * (edS @ (k * k) + (dS * dS) @ ek)
        else:
            edq = sc * sc * (edS0 @ (k * k) + (dS * dS) @ ek + edelta * (P @ k) ** 2)
        dk = dS.transpose(-1, -2) @ q * sc
        edk = sc * sc * (edS.transpose(-1, -2) @ (q * q) + (dS * dS).transpose(-1, -2) @ eq)
        dv = Pd.transpose(-1, -2) @ g
        edv = ePd.transpose(-1, -2) @ (g * g) + (Pd * Pd).transpose(-1, -2) @ eg
        # the part of each variance that comes from this kernel's own roundings (independent from row to row); the rest is inherited
        # from dctx, q, k, v, whose errors the attention spreads over the rows of a batch element: CORRELATED from row to row
        r2 = (U9 * dS) ** 2
        own = (sc * sc * (r2 @ (k * k)), sc * sc * (r2.transpose(-1, -2) @ (q * q)), ((U9 * Pd) ** 2).transpose(-1, -2) @ (g * g))
        self.inh = tuple(_rows((t - o).clamp_min(0.0)) for t, o in zip((edq, edk, edv), own))
        return tuple(ar.store(Q(_rows(a), _rows(b))) for a, b in ((dq, edq), (dk, edk), (dv, edv)))


def _flat(qq):
    return Q(qq.v.reshape(-1, qq.v.shape[-1]), qq.e.reshape(-1, qq.e.shape[-1]) if qq.e is not None else None)


def _unflat(qq, B):
    return Q(qq.v.reshape(B, -1, qq.v.shape[-1]), qq.e.reshape(B, -1, qq.e.shape[-1]) if qq.e is not None else None)


def _mask(keep, p):
    """keep / (1 - p) as an fp64 [M, H] factor; 1.0 without dropout."""
    if keep is None or p <= 0:
        return None
    return keep.reshape(-1, keep.shape[-1]).double() * float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))


class _Stream:
    """The blocks of one data stream of a layer behind its attention: proj (dense + dropout + residual + LayerNorm), FFN, and their
    backward.  All tensors [M, width]."""

    def __init__(self, ar, w, names, r32, keep_proj, keep_ffn, p):
        self.ar, self.n, self.r32, self.p = ar, names, r32, p
        self.W = lambda k: w[names[k] + ".weight"].double()
        self.b = lambda k: w[names[k] + ".bias"].double()
        self.kp, self.kf = _mask(keep_proj, p), _mask(keep_ffn, p)
        self.g = {}

    def _sum(self, lin, res, km):
        ar = self.ar
        if km is not None:
            lin = ar.scale(lin, km)
        s = ar.add(lin, res)
        return ar.store32(s) if self.r32 else ar.store(s)

    def _norm(self, s, ln):
        ar = self.ar
        y32, xh, r = _ln_fwd(ar, s, self.W(ln), self.b(ln))
        y = ar.store(y32)
        return y, (ar.store32(y32) if self.r32 else y), xh, r

    def fwd(self, ctx, x, x_res, ctx_inh=None):
        """ctx [M, Hb] (stored), x the layer input (bf16), x_res what the engine adds as the residual.  Returns y (stored bf16)."""
        ar = self.ar
        self.ctx, self.x, self.ctx_inh = ctx, x, ctx_inh
        s1 = self._sum(ar.lin(ctx, self.W("o"), self.b("o")), x_res, self.kp)
        self.a, a_res, self.xh1, self.r1 = self._norm(s1, "ln1")
        acc = ar.lin(self.a, self.W("up"), self.b("up"))
        self.u = ar.store(acc)
        gd = _gelu_d(acc.v)
        self.h = ar.store(Q(_gelu(acc.v), acc.e * gd * gd if ar.bound else None))
        if ar.mutate == "ffn_residual_from_layer_input":
            a_res = x_res
        s2 = self._sum(ar.lin(self.h, self.W("down"), self.b("down")), a_res, self.kf)
        y, _, self.xh2, self.r2 = self._norm(s2, "ln2")
        return y

    def _ln_back(self, g, xh, r, ln, km, bias_name):
        ar = self.ar
        dres32, dg, db = _ln_bwd(ar, g, xh, r, self.W(ln))
        self.g[self.n[ln] + ".weight"], self.g[self.n[ln] + ".bias"] = dg, db
        dres = ar.store(dres32)
        dl32 = dres32 if km is None else ar.scale(dres32, km)
        dl = dres if km is None else ar.store(dl32)
        self.g[self.n[bias_name] + ".bias"] = ar.colsum(dl32)            # the kernel adds its fp32 row values (adl)
        return dres, dl

    def bwd(self, g):
        """g = gradient of y (bf16).  Returns (dctx, dres_b): the attention context's gradient and the residual path's."""
        ar, n = self.ar, self.n
        last = (g.v.shape[0] - 1) if ar.mutate == "bias_grad_drops_last_row" else None
        dres_a, dl = self._ln_back(g, self.xh2, self.r2, "ln2", self.kf, "down")
        self.g[n["down"] + ".weight"] = ar.wgrad(dl, self.h)
        lin = ar.dgrad(dl, self.W("down"))
        gd = _gelu_d(self.u.v)
        du = Q(lin.v * gd, lin.e * gd * gd + (lin.v * _gelu_dd(self.u.v)) ** 2 * self.u.e if ar.bound else None)
        du = ar.store(du)
        self.g[n["up"] + ".weight"] = ar.wgrad(du, self.a)
        self.g[n["up"] + ".bias"] = ar.colsum(du, last)
        gc = ar.store(ar.add(ar.dgrad(du, self.W("up")), dres_a))
        dres_b, dl2 = self._ln_back(gc, self.xh1, self.r1, "ln1", self.kp, "o")
        self.g[n["o"] + ".weight"] = ar.wgrad(dl2, self.ctx, x_inh=self.ctx_inh)
        return ar.store(ar.dgrad(dl2, self.W("o"))), dres_b

    def qkv_bwd(self, dqkv, Wqkv, dres_b, inh=None):
        """dqkv [M, 3 Hb] (stored): the QKV parameter gradients and gx = dqkv W_qkv + dres_b.  inh [B, L, 3 Hb]: the part of dqkv's
        variance whose errors are correlated over the rows of a batch element (_Attn.bwd, _Ar.wgrad)."""
        ar, n = self.ar, self.n
        Hb = dqkv.v.shape[-1] // 3
        last = (dqkv.v.shape[0] - 1) if ar.mutate == "bias_grad_drops_last_row" else None
        dW, db = ar.wgrad(dqkv, self.x, dy_inh=inh), ar.colsum(dqkv, last, inh=inh)
        for j, k in enumerate("qkv"):
            src = 2 if (k == "k" and ar.mutate == "k_wgrad_from_v_slice") else j
            self.g[n[k] + ".weight"] = Q(dW.v[src * Hb:(src + 1) * Hb], dW.e[src * Hb:(src + 1) * Hb] if ar.bound else None)
            self.g[n[k] + ".bias"] = Q(db.v[j * Hb:(j + 1) * Hb], db.e[j * Hb:(j + 1) * Hb] if ar.bound else None)
        gx = ar.dgrad(dqkv, Wqkv)
        if ar.mutate != "dx_without_residual_path":
            gx = ar.add(gx, dres_b)
        return ar.store(gx)


def _cat(ar, qs):
    return Q(torch.cat([t.v for t in qs], -1), torch.cat([t.e for t in qs], -1) if ar.bound else None)


def _third(ar, t, j):
    H = t.v.shape[-1] // 3
    return Q(t.v[..., j * H:(j + 1) * H], t.e[..., j * H:(j + 1) * H] if ar.bound else None)


def _stale(ar, dy, dy_prev):
    """stale_gradient_tile: the first 32 x 32 tile of the [M, H] upstream gradient still holds the previous step's values."""
    if ar.mutate != "stale_gradient_tile":
        return dy
    d = dy.clone().reshape(-1, dy.shape[-1])
    d[:32, :32] = dy_prev.reshape(-1, dy.shape[-1])[:32, :32]
    return d.reshape(dy.shape)


def _off_by_one(ar, drops, key):
    if ar.mutate == "dropout_site_off_by_one" and drops:
        return drops.get(key + "_next", torch.roll(drops[key], 1, -1))
    return drops[key] if drops else None


def _run(ar, kind, sd, pre, cfg, x, dy, km, drops, p, r32, x32, dy_prev):
    w = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    x32 = x32 if isinstance(x32, tuple) else (x32, x32)                     # connection layer: (visual, text)
    rel_v, rel_t = (U9 if (r32 and f) else 0.0 for f in x32)
    res_rel = rel_v
    out = {}
    if kind != "c":
        B = x.shape[0]
        heads = cfg.num_attention_heads if kind == "t" else cfg.v_num_attention_heads
        if ar.mutate == "keymask_previous_row":
            km = torch.roll(torch.as_tensor(km), 1, 0)
        st = _Stream(ar, w, SELF, r32, drops["proj"] if drops else None, _off_by_one(ar, drops, "ffn"), p)
        xq = ar.exact(x)
        Wqkv = torch.cat([w[SELF[k] + ".weight"].double() for k in "qkv"], 0)
        bqkv = torch.cat([w[SELF[k] + ".bias"].double() for k in "qkv"], 0)
        qkv = ar.store(ar.lin(xq, Wqkv, bqkv))
        att = _Attn(ar, _third(ar, qkv, 0), _third(ar, qkv, 1), _third(ar, qkv, 2), km, heads, drops["attn"] if drops else None, p)
        ctx = att.fwd()
        y = st.fwd(_flat(ctx), _flat(xq), _flat(ar.exact(x, res_rel)), att.inh_ctx if ar.bound else None)
        dctx, dres_b = st.bwd(_flat(ar.exact(_stale(ar, dy, dy_prev))))
        dqkv = _cat(ar, att.bwd(_unflat(dctx, B)))
        inh = torch.cat(att.inh, -1) if ar.bound else None
        out["y"], out["gx"] = _unflat(y, B), _unflat(st.qkv_bwd(_flat(dqkv), Wqkv, dres_b, inh), B)
        out.update(st.g)
        return out
    (xv, xt), (dyv, dyt), (km_v, km_t) = x, dy, km
    B, V, T = xv.shape[0], xv.shape[1], xt.shape[1]
    heads = cfg.bi_num_attention_heads
    sv = _Stream(ar, w, CONN_V, r32, drops["proj_v"] if drops else None, _off_by_one(ar, drops, "ffn_v"), p)
    stt = _Stream(ar, w, CONN_T, r32, drops["proj_t"] if drops else None, drops["ffn_t"] if drops else None, p)
    qv, qt = ar.exact(xv), ar.exact(xt)
    Wq, qkv = {}, {}
    for nm, names, xq in (("v", CONN_V, qv), ("t", CONN_T, qt)):
        Wq[nm] = torch.cat([w[names[k] + ".weight"].double() for k in "qkv"], 0)
        qkv[nm] = ar.store(ar.lin(xq, Wq[nm], torch.cat([w[names[k] + ".bias"].double() for k in "qkv"], 0)))
    km_for_t = km_v                                                          # text queries attend to the visual keys
    if ar.mutate == "conn_wrong_keymask":
        km_for_t = torch.as_tensor(km_t)[:, :V]
    # ctx1 = attention(q2, k1, v1) [B, T, Hb] for the text stream, ctx2 = attention(q1, k2, v2) [B, V, Hb] for the visual stream
    a1 = _Attn(ar, _third(ar, qkv["t"], 0), _third(ar, qkv["v"], 1), _third(ar, qkv["v"], 2), km_for_t, heads, drops["attn_t"] if drops else None, p)
    a2 = _Attn(ar, _third(ar, qkv["v"], 0), _third(ar, qkv["t"], 1), _third(ar, qkv["t"], 2), km_t, heads, drops["attn_v"] if drops else None, p)
    ctx1, ctx2 = a1.fwd(), a2.fwd()
    if ar.mutate == "conn_ctx_swapped":
        ctx1, ctx2 = ctx2, ctx1
    yv = sv.fwd(_flat(ctx2), _flat(qv), _flat(ar.exact(xv, rel_v)), a2.inh_ctx if ar.bound else None)
    yt = stt.fwd(_flat(ctx1), _flat(qt), _flat(ar.exact(xt, rel_t)), a1.inh_ctx if ar.bound else None)
    prev = dy_prev if dy_prev is not None else (None, None)
    dctx2, dres_v = sv.bwd(_flat(ar.exact(_stale(ar, dyv, prev[0]))))
    dctx1, dres_t = stt.bwd(_flat(ar.exact(dyt)))
    if ar.mutate == "conn_ctx_swapped":
        dctx1, dctx2 = dctx2, dctx1
    dq2, dk1, dv1 = a1.bwd(_unflat(dctx1, B))
    dq1, dk2, dv2 = a2.bwd(_unflat(dctx2, B))
    out["y_v"], out["y_t"] = _unflat(yv, B), _unflat(yt, B)
    inh_v = torch.cat((a2.inh[0], a1.inh[1], a1.inh[2]), -1) if ar.bound else None
    inh_t = torch.cat((a1.inh[0], a2.inh[1], a2.inh[2]), -1) if ar.bound else None
    out["gx_v"] = _unflat(sv.qkv_bwd(_flat(_cat(ar, (dq1, dk1, dv1))), Wq["v"], dres_v, inh_v), B)
    out["gx_t"] = _unflat(stt.qkv_bwd(_flat(_cat(ar, (dq2, dk2, dv2))), Wq["t"], dres_t, inh_t), B)
    out.update(sv.g)
    out.update(stt.g)
    return out


def emulate(kind, sd, pre, cfg, x, dy, km, drops=None, p=0.0, r32=True, mutate=None, acc=torch.float64, dy_prev=None):
    """The same step with the engine's roundings (module docstring); arguments as `reference`.  r32: CrctStepCfg.residual_fp32.  The layer
    input's residual is the bf16 x itself (the emulator has no fp32 copy).  acc=torch.float32 runs the matmuls and reductions in fp32.
    mutate: one of MUTANTS --
      ffn_residual_from_layer_input   the FFN block adds the layer input instead of the attention block's output
      conn_ctx_swapped                the text stream's projection reads ctx2, the visual stream's ctx1 (T == V only)
      conn_wrong_keymask              the text-query attention masks with the first V columns of the TEXT key mask (T >= V)
      keymask_previous_row            batch row b of a self layer uses the key mask of row b - 1
      k_wgrad_from_v_slice            the K weight gradient comes from the dv third of dqkv
      dx_without_residual_path        gx = dqkv W_qkv without the dres_b addend
      bias_grad_drops_last_row        the QKV and FFN-up bias gradients sum M - 1 rows
      dropout_site_off_by_one         the FFN-output dropout (visual stream in a connection layer) uses another site's mask
                                      (drops["ffn_next"] / ["ffn_v_next"], else the mask rolled by one column); p > 0 only
      stale_gradient_tile             the first 32 x 32 tile of the upstream gradient (visual in a connection layer) comes from dy_prev"""
    assert mutate is None or mutate in MUTANTS
    out = _run(_Ar(False, acc, mutate), kind, sd, pre, cfg, x, dy, km, drops if p > 0 else None, p, r32, False, dy_prev)
    return {k: v.v for k, v in out.items()}


def budget(kind, sd, pre, cfg, x, dy, km, drops=None, p=0.0, r32=True, x32=True, coherent_delta=True):
    """Per-element budget of every output of the step (the stored output's own bf16 step excluded: `ratio` adds it), from the inputs and
    fp64 quantities alone.  x32: the engine adds an fp32 copy of the layer input as the residual (every layer input except the
    embeddings' outputs, under r32); a connection layer takes (visual, text).
    coherent_delta=False is the tighter form that adds the error of the attention backward's delta_i into dq in quadrature over the keys;
    tests/test_layer_ref_cpu.py::test_delta_error_reaches_dq_as_one_number shows the clean emulator outside it on real hidden states."""
    out = _run(_Ar(True, independent_delta=not coherent_delta), kind, sd, pre, cfg, x, dy, km, drops if p > 0 else None, p, r32, x32, None)
    own = lambda k, v: (U9 * v.v) ** 2 if stored_bf16(k) else 0.0
    return {k: KSIGMA * torch.sqrt((v.e - own(k, v)).clamp_min(0.0)) for k, v in out.items()}


# ------------------------------------------------------------------------------------------- the two embeddings (last segment)
# What the engine reads (engine.cpp embed_text_fwd / embed_image_fwd, rowops.hip): every table, the location Linears and the LayerNorm
# parameters from the fp32 masters; only the image Linear's matrix from the bf16 shadow (its bias from the masters).  Where it stores bf16:
# the softmax of the features, the image Linear's output, the pre-LayerNorm sum of both embeddings -- the norm is taken over exactly that
# rounded row -- and the outputs; backward: d_sum for the image Linear's weight gradient.  Every table / bias / location gradient adds the
# kernel's fp32 d_sum rows.
ET, EV = "bert.embeddings.", "bert.v_embeddings."


def embed_weights_of(table, flat_params, flat_shadow):
    sd = {}
    for e in table:
        if e.name.startswith((ET, EV)) and e.used and e.numel > 0:
            src = flat_shadow if e.name == EV + "new_image_embeddings.weight" else flat_params
            sd[e.name] = src[e.offset:e.offset + e.numel].detach().double().cpu().view(*e.shape)
    return sd


def reference_embed(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0):
    """O.embed_text / O.embed_image in fp64 under autograd.  batch: tokens, segments, loc, image_feat, image_loc, image_target;
    drops: {"t": keep [B, T, H], "v": keep [B, V, Hv]}.  Returns y_t, y_v and the gradient of every parameter (full names)."""
    w = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    saved = O._drop
    if p > 0:
        O._drop = _MaskDrop([drops["t"], drops["v"]], p)
    try:
        yt = O.embed_text(w, cfg, batch["tokens"], batch["segments"], batch["loc"].double(), p > 0)
        yv = O.embed_image(w, cfg, batch["image_feat"].double(), batch["image_loc"].double(), batch["image_target"], p > 0)
        torch.autograd.backward([yt, yv], [dy_t.double(), dy_v.double()])
    finally:
        O._drop = saved
    out = dict(y_t=yt.detach(), y_v=yv.detach())
    out.update({k: v.grad for k, v in w.items() if v.grad is not None})
    return out


def _scatter(ar, rows, idx, n, sel):
    """table gradient [n, H]: the fp32 rows `rows` [M, H] with sel added at their indices."""
    i = idx[sel]
    v = torch.zeros(n, rows.v.shape[-1], dtype=torch.float64).index_add_(0, i, rows.v[sel])
    if not ar.bound:
        return Q(v.to(torch.float32).double())
    e = torch.zeros_like(v).index_add_(0, i, rows.e[sel]) + S32 ** 2 * torch.zeros_like(v).index_add_(0, i, rows.v[sel] ** 2)
    return Q(v, e)


def _embed_side(ar, terms, g, b, keep, p, dy):
    """sum -> bf16, LayerNorm over the rounded row, dropout; backward rows in fp32.  Returns y [M, H] (stored), d_sum (fp32), dgamma, dbeta."""
    return _embed_side_q(ar, Q(terms, torch.zeros_like(terms) if ar.bound else None), g, b, keep, p, dy)


def _run_embed(ar, sd, cfg, batch, dy_t, dy_v, drops, p):
    out = {}
    W = lambda k: sd[k].double()
    # ---- text (vilbert.py:320-358 as O.embed_text states it)
    ids, segs, loc = batch["tokens"], batch["segments"], batch["loc"].double()
    B, T = ids.shape
    not_qa = (segs != -1) & (segs != 1)
    pos = torch.arange(T).unsqueeze(0).expand(B, T).clone()
    pos[not_qa] = T
    pos = pos - pos.min(dim=-1)[0].unsqueeze(1)
    pos[not_qa] = 0
    tt = segs.clone()
    tt[tt == -1] = 0
    has_loc = loc.abs().sum(-1) != 0
    locm = (loc * has_loc.unsqueeze(-1)).reshape(B * T, 4)
    terms = (W(ET + "word_embeddings.weight")[ids] + W(ET + "position_embeddings.weight")[pos] * (~not_qa).unsqueeze(-1) +
             W(ET + "plotqa_type_embeddings.weight")[tt] * (segs != 0).unsqueeze(-1) +
             (loc @ W(ET + "txt_location_embeddings.weight").t() + W(ET + "txt_location_embeddings.bias")) * has_loc.unsqueeze(-1))
    H = terms.shape[-1]
    y, ds, dg, db = _embed_side(ar, terms.reshape(B * T, H), W(ET + "LayerNorm.weight"), W(ET + "LayerNorm.bias"),
                                drops["t"] if drops else None, p, dy_t)
    rows = torch.ones(B * T, dtype=torch.bool)
    if ar.mutate == "embed_scatter_drops_last_row":
        rows[-1] = False
    out["y_t"] = _unflat(y, B)
    out[ET + "LayerNorm.weight"], out[ET + "LayerNorm.bias"] = dg, db
    out[ET + "word_embeddings.weight"] = _scatter(ar, ds, ids.flatten(), sd[ET + "word_embeddings.weight"].shape[0], rows)
    out[ET + "position_embeddings.weight"] = _scatter(ar, ds, pos.flatten(), sd[ET + "position_embeddings.weight"].shape[0], rows & ~not_qa.flatten())
    out[ET + "plotqa_type_embeddings.weight"] = _scatter(ar, ds, tt.flatten(), sd[ET + "plotqa_type_embeddings.weight"].shape[0], rows & (segs != 0).flatten())
    hl = has_loc.flatten().double().unsqueeze(-1)
    out[ET + "txt_location_embeddings.weight"] = ar.wgrad(ds, Q(locm, torch.zeros_like(locm) if ar.bound else None))
    out[ET + "txt_location_embeddings.bias"] = ar.colsum(ds if ar.mutate == "embed_loc_mask_ignored" else ar.scale(ds, hl))
    # ---- image (vilbert.py:1474-1496 as O.embed_image states it)
    feat, vloc, tgt = batch["image_feat"].double(), batch["image_loc"].double(), batch["image_target"]
    V = feat.shape[1]
    M = B * V
    sm = torch.softmax(feat, -1).reshape(M, -1)
    soft = ar.store(Q(sm, (S32 * sm) ** 2 if ar.bound else None))
    lin = ar.store(ar.lin(soft, W(EV + "new_image_embeddings.weight"), W(EV + "new_image_embeddings.bias")))
    rest = (vloc @ W(EV + "new_loc_emb.weight").t() + W(EV + "new_loc_emb.bias") + W(EV + "color_emb.weight")[tgt]).reshape(M, -1)
    terms = ar.add(lin, Q(rest, torch.zeros_like(rest) if ar.bound else None))
    y, ds, dg, db = _embed_side_q(ar, terms, W(EV + "LayerNorm.weight"), W(EV + "LayerNorm.bias"), drops["v"] if drops else None, p, dy_v)
    out["y_v"] = _unflat(y, B)
    out[EV + "LayerNorm.weight"], out[EV + "LayerNorm.bias"] = dg, db
    vl = vloc.reshape(M, 4)
    out[EV + "new_image_embeddings.weight"] = ar.wgrad(ar.store(ds), soft)
    out[EV + "new_image_embeddings.bias"] = ar.colsum(ds)
    out[EV + "new_loc_emb.bias"] = ar.colsum(ds)
    out[EV + "new_loc_emb.weight"] = ar.wgrad(ds, Q(vl, torch.zeros_like(vl) if ar.bound else None))
    vrows = torch.ones(M, dtype=torch.bool)
    if ar.mutate == "embed_scatter_drops_last_row":
        vrows[-1] = False
    out[EV + "color_emb.weight"] = _scatter(ar, ds, tgt.flatten(), sd[EV + "color_emb.weight"].shape[0], vrows)
    return out


def _embed_side_q(ar, s, g, b, keep, p, dy):
    """_embed_side for a sum that already carries a variance (the image Linear's output)."""
    s = ar.store(s)
    km = _mask(keep, p)
    y32, xh, r = _ln_fwd(ar, s, g, b)
    y = ar.store(y32 if km is None else ar.scale(y32, km))
    dyq = _flat(ar.exact(dy))
    dsum, dg, db = _ln_bwd(ar, dyq if km is None else ar.scale(dyq, km), xh, r, g)
    return y, dsum, dg, db


def emulate_embed(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0, mutate=None, acc=torch.float64):
    """The embeddings with the engine's roundings.  mutate (EMBED_MUTANTS): embed_scatter_drops_last_row -- the last token / element is
    missing from the table gradients; embed_loc_mask_ignored -- the text location bias sums the rows without a box too."""
    assert mutate is None or mutate in EMBED_MUTANTS
    return {k: v.v for k, v in _run_embed(_Ar(False, acc, mutate), sd, cfg, batch, dy_t, dy_v, drops if p > 0 else None, p).items()}


def budget_embed(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0):
    out = _run_embed(_Ar(True), sd, cfg, batch, dy_t, dy_v, drops if p > 0 else None, p)
    own = lambda k, v: (U9 * v.v) ** 2 if stored_bf16(k) else 0.0
    return {k: KSIGMA * torch.sqrt((v.e - own(k, v)).clamp_min(0.0)) for k, v in out.items()}


# ------------------------------------------------------------------------------------------- heads plus losses (segment 0)
# What the engine reads (engine.cpp heads_branch_fwd / heads_tail_fwd / heads_bwd, heads.hip): the matrices of the two poolers, the two
# regressor pipes and fusion.0 / .2 / .4 from the bf16 shadow; cls.bi_seq_relationship and fusion.6 -- the head kernel's -- and every
# bias from the fp32 masters.  Where it stores bf16: the poolers' outputs, every pipe / fusion activation (post-LeakyReLU) and the pipes'
# last outputs (cat); backward: the head kernel's seeds d_pooled_t / d_pooled_v / d_fus_h, every gradient buffer of the chain, and the
# CLS / IMG rows of the hidden gradients, which the pooler's data gradient writes and the pipe's then adds to (two roundings).  The head
# kernel itself (fused product, cls dropout, logits, tanh, losses, its four parameter gradients) works in fp32.  The bias gradients are
# column sums of the bf16 gradient buffers.  An activation derivative is read off the stored post-activation's sign: a pre-activation
# within its own budget of zero may take either slope, which the budget carries as the full step between the two.
HEAD_LINEARS = (["bert.t_pooler.dense", "bert.v_pooler.dense", "cls.bi_seq_relationship"] +
                ["regressor.%s.%d" % (n, j) for n in ("txt_pipe", "vis_pipe", "fusion") for j in (0, 2, 4, 6)])
HEAD_FP32_MATRICES = ("cls.bi_seq_relationship.weight", "regressor.fusion.6.weight")


def head_weights_of(table, flat_params, flat_shadow):
    sd = {}
    for e in table:
        if e.name.rsplit(".", 1)[0] in HEAD_LINEARS and e.used and e.numel > 0:
            src = flat_shadow if (len(e.shape) == 2 and e.name not in HEAD_FP32_MATRICES) else flat_params
            sd[e.name] = src[e.offset:e.offset + e.numel].detach().double().cpu().view(*e.shape)
    return sd


def reference_heads(sd, cfg, params, seq_t, seq_v, R, labels, keep=None, p=0.0):
    """O.heads_and_losses in fp64 under autograd on the full hidden states (training step: kind "L1_smooth"), loss = nsp_loss_coeff nsp +
    reg_loss_coeff mean_B reg_loss.  keep: the engine's cls dropout mask [B, Hb].  Returns logits, reg_pred, reg_loss, reg_l1, loss, nsp,
    gx_t / gx_v (the whole hidden gradients [B, L, H]: rows 1.. are zero) and every head parameter gradient."""
    w = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    xt, xv = (t.detach().double().clone().requires_grad_(True) for t in (seq_t, seq_v))
    saved = O._drop
    if p > 0:
        O._drop = _MaskDrop([keep], p)
    try:
        logits, reg, nsp, r = O.heads_and_losses(w, cfg, params, xt, xv, R.double(), "L1_smooth", labels, p > 0, p)
        loss = (params["nsp_loss_coeff"] * nsp + params["reg_loss_coeff"] * reg[1].mean()).sum()
        loss.backward()
    finally:
        O._drop = saved
    out = dict(logits=logits.detach(), reg_pred=reg[0].detach(), reg_loss=reg[1].detach(), reg_l1=reg[2].detach(), loss=loss.detach().reshape(1),
               nsp=nsp.detach().reshape(1), gx_t=xt.grad, gx_v=xv.grad)
    out.update({k: v.grad for k, v in w.items() if v.grad is not None})
    return out


def _qz(ar, v):
    return Q(v, torch.zeros_like(v) if ar.bound else None)


def _act_fwd(ar, acc, kind):
    """post-activation of the fp32 accumulator, stored bf16 ("relu" / "leaky" / None)."""
    if kind is None:
        return ar.store(acc)
    sl = torch.where(acc.v > 0, 1.0, 0.0 if kind == "relu" else 0.01)
    if not ar.bound:
        return ar.store(Q(acc.v * sl))
    near = acc.v.abs() <= KSIGMA * torch.sqrt(acc.e)                     # the engine's accumulator may lie on the other side of the kink
    return ar.store(Q(acc.v * sl, acc.e * torch.where(near, torch.ones_like(sl), sl * sl)))


def _act_bwd(ar, g, a, kind):
    """g times the activation's derivative, read off the stored post-activation a."""
    if kind is None:
        return g
    lo = 0.0 if kind == "relu" else 0.01
    sl = torch.where(a.v > 0, 1.0, lo)
    if not ar.bound:
        return Q(g.v * sl)
    # strictly inside: a dead ReLU unit is stored as 0 with variance 0 and is NOT in doubt; one near the kink carries the accumulator's
    # variance (_act_fwd)
    either = (a.v.abs() < KSIGMA * torch.sqrt(a.e)).double()           # may take either slope
    # ... entered as a deviation of the size of the step between the two slopes.  At the unit itself that is generous (KSIGMA steps); the
    # margin is needed further down, where the step arrives projected through weight matrices and sums over a few batch rows, and one
    # element among 10^5 ... 10^6 sits several of those projections' own deviations out.  (Entered as a bare step, without that margin, the
    # clean emulator read 1.73 on pipe weight gradients with the recorded hidden states of tests/golden/heads_rows_B3.npz; with it 0.37.)
    return Q(g.v * sl, g.e * sl * sl + either * ((1.0 - lo) * g.v) ** 2)


class _Chain:
    """Linear (+ activation) layers in a row with bf16 activations, and their backward as heads_bwd / pipe_bwd run it."""

    def __init__(self, ar, sd, names, kinds, grads):
        self.ar, self.sd, self.names, self.kinds, self.g = ar, sd, names, kinds, grads

    def fwd(self, x):
        self.x = [x]
        for n, k in zip(self.names, self.kinds):
            x = _act_fwd(self.ar, self.ar.lin(x, self.sd[n + ".weight"], self.sd[n + ".bias"]), k)
            self.x.append(x)
        return x

    def bwd(self, g, last_dgrad=True):
        """g: stored gradient of the last Linear's pre-activation.  Returns the data gradient of the input (fp32 accumulator, not stored)."""
        ar = self.ar
        for i in range(len(self.names) - 1, -1, -1):
            n = self.names[i]
            self.g[n + ".bias"] = ar.colsum(g)
            self.g[n + ".weight"] = ar.wgrad(g, self.x[i])
            if i == 0:
                return ar.dgrad(g, self.sd[n + ".weight"]) if last_dgrad else None
            g = ar.store(_act_bwd(ar, ar.dgrad(g, self.sd[n + ".weight"]), self.x[i], self.kinds[i - 1]))


def _run_heads(ar, sd, cfg, params, seq_t, seq_v, R, labels, keep, p):
    assert cfg.fusion_method == "mul"
    sd = {k: v.double() for k, v in sd.items()}
    B = seq_t.shape[0]
    g = {}
    xt, xv = ar.exact(seq_t[:, 0]), ar.exact(seq_v[:, 0])
    pool_t, pool_v = _Chain(ar, sd, ["bert.t_pooler.dense"], ["relu"], g), _Chain(ar, sd, ["bert.v_pooler.dense"], ["relu"], g)
    pipe = lambda n: _Chain(ar, sd, ["regressor.%s.%d" % (n, j) for j in (0, 2, 4, 6)], ["leaky", "leaky", "leaky", None], g)
    pipe_t, pipe_v = pipe("txt_pipe"), pipe("vis_pipe")
    fus = _Chain(ar, sd, ["regressor.fusion.%d" % j for j in (0, 2, 4)], ["leaky"] * 3, g)
    pt, pv, hw, hv = pool_t.fwd(xt), pool_v.fwd(xv), pipe_t.fwd(xt), pipe_v.fwd(xv)
    swap = ar.mutate == "heads_cat_halves_swapped"
    fh = fus.fwd(_cat(ar, (hw, hv) if swap else (hv, hw)))
    # ---- the head kernel (fp32): vilbert.py:1048-1062, :1583-1657 as O.heads_and_losses states them
    ks = (keep.double() * float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))) if p > 0 else torch.ones_like(pt.v)
    fd = Q(pt.v * pv.v * ks, (pt.e * pv.v ** 2 + pt.v ** 2 * pv.e) * ks * ks if ar.bound else None)
    Wc, W6 = sd["cls.bi_seq_relationship.weight"], sd["regressor.fusion.6.weight"]
    logits = ar.lin(fd, Wc, sd["cls.bi_seq_relationship.bias"])
    z = ar.lin(fh, W6, sd["regressor.fusion.6.bias"])
    r = torch.tanh(z.v).squeeze(-1)
    dr_dz = 1.0 - r * r
    er = (z.e.squeeze(-1) * dr_dz ** 2 + (S32 * r) ** 2) if ar.bound else None
    R = R.double()
    needs = R[:, 1] == 1
    target = R[:, 0] / torch.where(needs, R[:, 3], torch.ones_like(R[:, 3]))
    diff = r - target
    live = needs & ~(target.abs() > 1)                                   # rows whose regression loss counts (kind "L1_smooth")
    rl = torch.where(live, diff.abs() if params["L1"] else torch.where(diff.abs() < 0.5, diff * diff, diff.abs() - 0.25), torch.zeros_like(r))
    drl = torch.where(live, torch.sign(diff) if params["L1"] else torch.where(diff.abs() < 0.5, 2 * diff, torch.sign(diff)), torch.zeros_like(r))
    ddrl = torch.zeros_like(r) if params["L1"] else torch.where(live & (diff.abs() < 0.5), 2.0, 0.0)
    valid = labels.reshape(-1) != -1
    nv = max(int(valid.sum()), 1)
    lab = labels.reshape(-1).clamp_min(0)
    P2 = torch.softmax(logits.v, -1)
    ce = torch.where(valid, torch.logsumexp(logits.v, 1) - logits.v.gather(1, lab[:, None]).squeeze(1), torch.zeros_like(r))
    nsp = ce.sum() / nv
    cn, cr = float(params["nsp_loss_coeff"]), float(params["reg_loss_coeff"])
    dlog = (P2 - torch.nn.functional.one_hot(lab, 2).double()) * valid[:, None] * (cn / nv)
    g_reg = cr if ar.mutate == "heads_reg_seed_without_batch_mean" else cr / B
    out = {}
    f32 = (lambda v, e: Q(v, e + (S32 * v) ** 2)) if ar.bound else (lambda v, e: Q(v.to(torch.float32).double()))
    zl = lambda t: torch.zeros_like(t)
    out["logits"] = f32(logits.v, logits.e)
    out["reg_pred"] = f32(torch.where(needs, r * R[:, 3], zl(r)), er * torch.where(needs, R[:, 3] ** 2, zl(r)) if ar.bound else None)
    out["reg_loss"] = f32(rl, er * drl ** 2 if ar.bound else None)
    out["reg_l1"] = f32(torch.where(needs, diff.abs(), zl(r)), er * needs if ar.bound else None)
    e_nsp = ((dlog / cn) ** 2 * logits.e).sum() if ar.bound else None
    out["nsp"] = f32(nsp.reshape(1), e_nsp.reshape(1) if ar.bound else None)
    out["loss"] = f32((cn * nsp + cr * rl.sum() / B).reshape(1), (cn ** 2 * e_nsp + (cr / B) ** 2 * (er * drl ** 2).sum()).reshape(1) if ar.bound else None)
    # seeds
    pp = (P2[:, 0] * P2[:, 1])[:, None]
    dlq = Q(dlog, (((cn / nv) * pp) ** 2 * logits.e.sum(-1, keepdim=True) * valid[:, None]).expand(-1, 2) + (S32 * dlog) ** 2 if ar.bound else None)
    g["cls.bi_seq_relationship.weight"], g["cls.bi_seq_relationship.bias"] = ar.wgrad(dlq, fd), ar.colsum(dlq)
    dfd = ar.dgrad(dlq, Wc)
    dfu = ar.scale(dfd, ks)

    def pooled_seed(own, other):
        v = dfu.v * other.v
        return ar.store(_act_bwd(ar, Q(v, dfu.e * other.v ** 2 + dfu.v ** 2 * other.e if ar.bound else None), own, "relu"))
    d_pt, d_pv = pooled_seed(pt, pv), pooled_seed(pv, pt)
    dz_v = (g_reg * drl * dr_dz)[:, None]
    dz = Q(dz_v, ((g_reg * (ddrl * dr_dz ** 2 - drl * 2 * r * dr_dz)) ** 2)[:, None] * z.e + (S32 * dz_v) ** 2 if ar.bound else None)
    g["regressor.fusion.6.weight"], g["regressor.fusion.6.bias"] = ar.wgrad(dz, fh), ar.colsum(dz)
    g0 = ar.store(_act_bwd(ar, ar.dgrad(dz, W6), fh, "leaky"))
    # ---- the chain of heads_bwd: poolers write the CLS / IMG rows, fusion, then the pipes add to those rows
    row_t, row_v = ar.store(pool_t.bwd(d_pt)), ar.store(pool_v.bwd(d_pv))
    dcat = ar.store(fus.bwd(g0))
    half = lambda j: Q(dcat.v[:, 256 * j:256 * (j + 1)], dcat.e[:, 256 * j:256 * (j + 1)] if ar.bound else None)
    dv_, dt_ = pipe_v.bwd(half(1 if swap else 0)), pipe_t.bwd(half(0 if swap else 1))
    over = ar.mutate == "heads_pipe_row_overwrites_pooler_row"
    out["gx_t"] = ar.store(dt_ if over else ar.add(dt_, row_t))
    out["gx_v"] = ar.store(dv_ if over else ar.add(dv_, row_v))
    out.update(g)
    return out


def emulate_heads(sd, cfg, params, seq_t, seq_v, R, labels, keep=None, p=0.0, mutate=None, acc=torch.float64):
    """Segment 0 with the engine's roundings; gx_t / gx_v are the CLS / IMG rows [B, H].  mutate (HEAD_MUTANTS): heads_cat_halves_swapped --
    the fusion MLP reads (hw, hv) and hands the halves of d cat back accordingly; heads_reg_seed_without_batch_mean -- the regression
    seed misses 1 / B; heads_pipe_row_overwrites_pooler_row -- the pipe's input gradient replaces the pooler's row instead of adding to it."""
    assert mutate is None or mutate in HEAD_MUTANTS
    return {k: v.v for k, v in _run_heads(_Ar(False, acc, mutate), sd, cfg, params, seq_t, seq_v, R, labels, keep, p).items()}


def budget_heads(sd, cfg, params, seq_t, seq_v, R, labels, keep=None, p=0.0):
    out = _run_heads(_Ar(True), sd, cfg, params, seq_t, seq_v, R, labels, keep, p)
    own = lambda k, v: (U9 * v.v) ** 2 if stored_bf16(k) else 0.0
    return {k: KSIGMA * torch.sqrt((v.e - own(k, v)).clamp_min(0.0)) for k, v in out.items()}
