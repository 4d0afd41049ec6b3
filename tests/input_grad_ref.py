"""Host-only yardstick for the gradients of the step's FLOAT inputs (crct_engine_set_input_grads; csrc/rowops.hip embed_input_grad_kernel
and softmax_bwd_rows_kernel; engine.cpp embed_text_input_grads / embed_image_input_grads), in the manner of tests/layer_ref.py, whose
error algebra (_Ar, Q, KSIGMA) it uses: an fp64 truth, an emulator of the engine's arithmetic with named mutants, a per-element budget.

Three levels, each from its own inputs:
  softmax backward   d_x = s (g - <s, g>), s = softmax(x)                                        softmax_bwd_reference / _emulate / _budget
  the row kernel     d_sum from (dy, saved sum, mean, rstd, gamma, mask); d_loc, d_areas from it   rows_reference / _emulate / _budget
  the segment        both embeddings: image_feat, image_loc, areas, txt_loc and the summed text    reference_inputs / emulate_inputs /
                     embeddings, from the hidden gradients that enter the last backward segment    budget_inputs

What the engine rounds.  d_sum is the fp32 row of the embedding backward (layer_ref._ln_bwd over the bf16 saved sum); d_loc, d_areas and the
text-embedding gradient are fp32 sums / copies of it.  The features' gradient goes through the image Linear's data-gradient GEMM, which reads
the bf16 copy of d_sum and the bf16 matrix and leaves g in fp32, and then through the softmax backward in fp32 with s recomputed in fp32
from the raw features.  Nothing else is stored in between.

The budget of the softmax backward (the only new algebra; everything else is layer_ref's).  With e_g the incoming variance of g:
  s^2 (e_g + sum_k s_k^2 e_gk)              the errors of g, directly and through the mean <s, g>, in quadrature
  S32^2 s^2 sum_k (s_k g_k)^2               fp32 accumulation of <s, g> and independent relative errors of the s_k inside it
  S32^2 s^2 <s, g>^2                        the one relative error all s_k share (the row's 1 / sum exp), coherent in <s, g>
  (S32 d)^2                                 relative error of s_j itself and of the final product
so an element whose true value is far below one fp32 step of g_j -- the hot element of an almost one-hot row, where g_j - <s, g> cancels
-- is held to the fp32 resolution of <s, g>, not to its own size: no fp32 evaluation of that difference can do better.

Mutants (each a plausible wiring error; tests/test_input_grad_ref_cpu.py shows that each leaves the budget):
  softmax_bwd_no_mean          d_x = s g: the - s <s, g> term is missing
  txt_loc_mask_ignored         a text row without a box (|loc|_1 == 0) gets a location gradient
  input_grad_no_dropout_mask   d_sum is rebuilt without the keep mask (p > 0 only)
  areas_uses_loc_weight        d_areas is taken against the first column of the location Linear's matrix
"""
import torch

import layer_ref as LR
from layer_ref import ET, EV, F32, KSIGMA, Q, S32, _Ar
from oracle import crct_oracle as O

MUTANTS = ("softmax_bwd_no_mean", "txt_loc_mask_ignored", "input_grad_no_dropout_mask", "areas_uses_loc_weight")
EPS = O.LN_EPS


def ratio(got, ref, bud):
    """|got - ref| / budget per element (fp32 outputs: no storage step is added); 0 where both are the same number (exact zeros)."""
    got, ref = got.double().cpu().reshape(ref.shape), ref.double()
    r = (got - ref).abs() / bud.reshape(ref.shape)
    return torch.where(got == ref, torch.zeros_like(r), r)


def _out(ar, outs):
    if ar.bound:
        return {k: KSIGMA * torch.sqrt(v.e) for k, v in outs.items()}
    return {k: v.v for k, v in outs.items()}


# ------------------------------------------------------------------------------------------- softmax backward
def softmax_bwd_reference(x, g):
    xx = x.detach().double().clone().requires_grad_(True)
    torch.softmax(xx, -1).backward(g.double())
    return xx.grad


def _softmax_bwd(ar, x, g):
    """x [M, F] the raw features (exact: fp32, or bf16 values), g a Q [M, F].  Returns d_x as a Q (stored fp32)."""
    xv = x.detach().double()
    if ar.bound:
        s = torch.softmax(xv, -1)
        dot = (s * g.v).sum(-1, keepdim=True)
        d = s * (g.v - dot)
        e = s * s * (g.e + (s * s * g.e).sum(-1, keepdim=True) + S32 ** 2 * ((s * g.v) ** 2).sum(-1, keepdim=True) + (S32 * dot) ** 2)
        return Q(d, e + (S32 * d) ** 2 + (F32 * d) ** 2)
    s = torch.softmax(xv.to(torch.float32), -1)                     # the kernel's fp32 recomputation
    gv = g.v.to(torch.float32)
    if ar.mutate == "softmax_bwd_no_mean":
        return Q((s * gv).double())
    dot = (s.to(ar.acc) * gv.to(ar.acc)).sum(-1, keepdim=True).to(torch.float32)
    return Q((s * (gv - dot)).double())


def softmax_bwd_emulate(x, g, mutate=None, acc=torch.float64):
    ar = _Ar(False, acc, mutate)
    return _softmax_bwd(ar, x, ar.exact(g)).v


def softmax_bwd_budget(x, g):
    ar = _Ar(True)
    return KSIGMA * torch.sqrt(_softmax_bwd(ar, x, ar.exact(g)).e)


# ------------------------------------------------------------------------------------------- the row kernel from its own inputs
def row_stats(x):
    """(mean, rstd) fp32 [M] of the bf16 rows x as the embedding forward leaves them (fp32 statistics of the rounded row)."""
    v = x.to(torch.float32)
    mean = v.mean(-1)
    var = ((v - mean.unsqueeze(-1)) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + EPS)


def _dsum(ar, dy, x, mean, rstd, gamma, keep, p):
    """The LayerNorm-backward row from the kernel's inputs: dy, x [M, H] bf16 values, mean / rstd [M] the fp32 numbers handed to it."""
    dyq = ar.exact(dy)
    km = LR._mask(keep, p)
    if km is not None and ar.mutate != "input_grad_no_dropout_mask":
        dyq = ar.scale(dyq, km)
    r = rstd.detach().double().unsqueeze(-1)
    xh = (x.detach().double() - mean.detach().double().unsqueeze(-1)) * r
    if not ar.bound:
        xh = ((x.detach().to(ar.acc) - mean.detach().to(ar.acc).unsqueeze(-1)) * r.to(ar.acc)).double()
    xq = Q(xh, (S32 * xh) ** 2 if ar.bound else None)
    rq = Q(r, (F32 * r) ** 2 if ar.bound else None)
    return LR._ln_bwd(ar, dyq, xq, rq, gamma.detach().double())[0]


def _wsum(ar, ds, W, coh=None, stored=False):
    """d_sum W, W [H, N]: a sum over the COLUMNS of a LayerNorm-backward row.  stored: the GEMM reads the bf16 copy of d_sum.
    The errors d_sum inherits from the rounded pre-LayerNorm sum s are not independent from column to column -- the row's mean, rstd
    and the two means of the backward are each ONE number -- so that part is not added in quadrature over the columns but passed through
    the exact Jacobian of the row, d(d_sum) / d(s) = alpha I + sum_i u_i v_i^T (_side), before it is squared:
    var_f = sum_c e_c (alpha W_cf + sum_i (u_i . W_f) v_ic)^2.  Everything else (fp32 slack, the bf16 copy) is independent per element."""
    if stored:
        ds = ar.store(ds)
    out = ar.dgrad(ds, W)
    if ar.bound and coh is not None:
        e_s, alpha, us, vs = coh
        W2 = W * W
        B = [u @ W for u in us]
        var = (alpha * alpha * e_s) @ W2
        for i, v in enumerate(vs):
            var = var + 2.0 * B[i] * ((alpha * e_s * v) @ W)
            for j, v2 in enumerate(vs):
                var = var + B[i] * B[j] * (e_s * v * v2).sum(-1, keepdim=True)
        out = Q(out.v, out.e + var.clamp_min(0.0))
    return out


def _from_dsum(ar, ds, w_loc=None, loc=None, w_areas=None, coh=None):
    """d_loc = d_sum W_loc (rows without a box: zero, when loc is given), d_areas = d_sum w_areas, fp32 sums of the fp32 row."""
    out = {}
    if w_loc is not None:
        d = _wsum(ar, ds, w_loc.detach().double(), coh)
        if loc is not None and ar.mutate != "txt_loc_mask_ignored":
            d = ar.scale(d, (loc.detach().double().abs().sum(-1, keepdim=True) != 0).double())
        out["d_loc"] = ar.store32(d)
    if w_areas is not None:
        wa = w_loc.detach().double()[:, :1] if ar.mutate == "areas_uses_loc_weight" else w_areas.detach().double().reshape(-1, 1)
        out["d_areas"] = ar.store32(_wsum(ar, ds, wa, coh))
    return out


def _rows(ar, dy, x, mean, rstd, gamma, keep, p, w_loc, loc, w_areas):
    ds = _dsum(ar, dy, x, mean, rstd, gamma, keep if p > 0 else None, p)
    out = _from_dsum(ar, ds, w_loc, loc, w_areas)
    out["d_sum"] = ar.store32(ds)
    return out


def rows_reference(dy, x, mean, rstd, gamma, keep=None, p=0.0, w_loc=None, loc=None, w_areas=None):
    """fp64 from the kernel's own inputs: the formula of the LayerNorm backward with the statistics it is handed."""
    ar = _Ar(False, torch.float64)
    ds = _dsum(ar, dy, x, mean, rstd, gamma, keep if p > 0 else None, p)
    out = {"d_sum": ds.v}
    if w_loc is not None:
        out["d_loc"] = ds.v @ w_loc.double()
        if loc is not None:
            out["d_loc"] = out["d_loc"] * (loc.double().abs().sum(-1, keepdim=True) != 0)
    if w_areas is not None:
        out["d_areas"] = ds.v @ w_areas.double().reshape(-1, 1)
    return out


def rows_emulate(dy, x, mean, rstd, gamma, keep=None, p=0.0, w_loc=None, loc=None, w_areas=None, mutate=None, acc=torch.float32):
    return _out(_Ar(False, acc, mutate), _rows(_Ar(False, acc, mutate), dy, x, mean, rstd, gamma, keep, p, w_loc, loc, w_areas))


def rows_budget(dy, x, mean, rstd, gamma, keep=None, p=0.0, w_loc=None, loc=None, w_areas=None):
    return _out(_Ar(True), _rows(_Ar(True), dy, x, mean, rstd, gamma, keep, p, w_loc, loc, w_areas))


# ------------------------------------------------------------------------------------------- the embeddings segment
def _image_variant(w, cfg, loc, target, areas, training):
    """BertImageEmbeddings.forward for 'dvqa' / 'figure_qa' (vilbert.py:1474-1489): no feature term, areas_emp(areas) when areas are given."""
    e = O.linear(w, EV + "new_loc_emb", loc) + w[EV + "color_emb.weight"][target]
    if areas is not None:
        e = e + O.linear(w, EV + "areas_emp", areas)
    e = O.layer_norm(e, w[EV + "LayerNorm.weight"], w[EV + "LayerNorm.bias"])
    return O._drop(e, cfg.hidden_dropout_prob, training)


def reference_inputs(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0, feat=True):
    """O.embed_text / O.embed_image in fp64 under autograd with the float inputs requiring grad (feat=False: the variants' image embedding,
    batch["areas"] [B, V, 1] optional).  Returns image_feat (feat only), image_loc, areas (when given), txt_loc and text_emb -- the gradient
    of the summed text embeddings, caught at the input of the text LayerNorm."""
    w = {k: v.detach().double() for k, v in sd.items()}
    f = lambda t: t.detach().double().clone().requires_grad_(True)
    tloc, vloc = f(batch["loc"]), f(batch["image_loc"])
    feats = f(batch["image_feat"]) if feat else None
    areas = f(batch["areas"]) if (not feat and batch.get("areas") is not None) else None
    seen = []
    saved_drop, saved_ln = O._drop, O.layer_norm

    def ln(x, g, b):
        x.retain_grad()
        seen.append(x)
        return saved_ln(x, g, b)
    O.layer_norm = ln
    if p > 0:
        O._drop = LR._MaskDrop([drops["t"], drops["v"]], p)
    try:
        yt = O.embed_text(w, cfg, batch["tokens"], batch["segments"], tloc, p > 0)
        yv = (O.embed_image(w, cfg, feats, vloc, batch["image_target"], p > 0) if feat else
              _image_variant(w, cfg, vloc, batch["image_target"], areas, p > 0))
        torch.autograd.backward([yt, yv], [dy_t.double(), dy_v.double()])
    finally:
        O._drop, O.layer_norm = saved_drop, saved_ln
    out = dict(txt_loc=tloc.grad, image_loc=vloc.grad, text_emb=seen[0].grad)
    if feat:
        out["image_feat"] = feats.grad
    if areas is not None:
        out["areas"] = areas.grad
    return out


def _side(ar, s, g, b, keep, p, dy):
    """layer_ref._embed_side_q with the backward's mask open to the mutant.  Returns (d_sum, d_sum_own, coh): the fp32 row [M, H] with
    its per-element variance (what a copy of the row carries); and, for sums over its columns (_wsum), the row with the variance of its
    own fp32 arithmetic alone plus coh = (e_s, alpha, (u_i), (v_i)), the variance of the stored sum s and the Jacobian of the row with
    respect to s.  With a = dy mask gamma, m2 = mean(a xhat) and d_sum = r (a - mean(a) - xhat m2), a change eps of s moves
    d_sum by -r^2 m2 eps + (r^2 m2 / H) 1 (1 . eps) + ((r^2 m2 / H) xhat - (r / H) d_sum) (xhat . eps) - (r / H) xhat (d_sum . eps)."""
    s = ar.store(s)
    km = LR._mask(keep, p)
    _, xh, r = LR._ln_fwd(ar, s, g, b)
    dyq = LR._flat(ar.exact(dy))
    if km is not None and ar.mutate != "input_grad_no_dropout_mask":
        dyq = ar.scale(dyq, km)
    ds = LR._ln_bwd(ar, dyq, xh, r, g)[0]
    if not ar.bound:
        return ds, ds, None
    _, xh0, r0 = LR._ln_fwd(ar, Q(s.v, torch.zeros_like(s.v)), g, b)
    own = LR._ln_bwd(ar, dyq, xh0, r0, g)[0]
    H = s.v.shape[-1]
    m2 = (dyq.v * g * xh.v).mean(-1, keepdim=True)
    rr = r.v
    us = (rr * rr * m2 / H * torch.ones_like(xh.v), rr * rr * m2 / H * xh.v - rr / H * ds.v, -rr / H * xh.v)
    vs = (torch.ones_like(xh.v), xh.v, ds.v)
    return ds, own, (s.e, -rr * rr * m2, us, vs)


def _run_inputs(ar, sd, cfg, batch, dy_t, dy_v, drops, p, feat):
    W = lambda k: sd[k].double()
    zero = lambda t: torch.zeros_like(t) if ar.bound else None
    out = {}
    # ---- text: the sum as layer_ref._run_embed builds it
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
    terms = (W(ET + "word_embeddings.weight")[ids] + W(ET + "position_embeddings.weight")[pos] * (~not_qa).unsqueeze(-1) +
             W(ET + "plotqa_type_embeddings.weight")[tt] * (segs != 0).unsqueeze(-1) +
             (loc @ W(ET + "txt_location_embeddings.weight").t() + W(ET + "txt_location_embeddings.bias")) * has_loc.unsqueeze(-1))
    terms = terms.reshape(B * T, -1)
    ds, own, coh = _side(ar, Q(terms, zero(terms)), W(ET + "LayerNorm.weight"), W(ET + "LayerNorm.bias"), drops["t"] if drops else None, p, dy_t)
    out["text_emb"] = LR._unflat(ar.store32(ds), B)
    out["txt_loc"] = LR._unflat(_from_dsum(ar, own, W(ET + "txt_location_embeddings.weight"), loc.reshape(B * T, 4), coh=coh)["d_loc"], B)
    # ---- image
    vloc, tgt = batch["image_loc"].double(), batch["image_target"]
    V = vloc.shape[1]
    M = B * V
    rest = (vloc @ W(EV + "new_loc_emb.weight").t() + W(EV + "new_loc_emb.bias") + W(EV + "color_emb.weight")[tgt]).reshape(M, -1)
    areas = batch.get("areas") if not feat else None
    if feat:
        featv = batch["image_feat"].double().reshape(M, -1)
        sm = torch.softmax(featv, -1)
        soft = ar.store(Q(sm, (S32 * sm) ** 2 if ar.bound else None))
        lin = ar.store(ar.lin(soft, W(EV + "new_image_embeddings.weight"), W(EV + "new_image_embeddings.bias")))
        terms = ar.add(lin, Q(rest, zero(rest)))
    else:
        if areas is not None:
            rest = rest + areas.double().reshape(M, 1) @ W(EV + "areas_emp.weight").t() + W(EV + "areas_emp.bias")
        terms = Q(rest, zero(rest))
    ds, own, coh = _side(ar, terms, W(EV + "LayerNorm.weight"), W(EV + "LayerNorm.bias"), drops["v"] if drops else None, p, dy_v)
    got = _from_dsum(ar, own, W(EV + "new_loc_emb.weight"), None, W(EV + "areas_emp.weight") if areas is not None else None, coh=coh)
    out["image_loc"] = LR._unflat(got["d_loc"], B)
    if areas is not None:
        out["areas"] = LR._unflat(got["d_areas"], B)
    if feat:
        g = ar.store32(_wsum(ar, own, W(EV + "new_image_embeddings.weight"), coh, stored=True))      # bf16 d_sum x bf16 matrix -> fp32
        out["image_feat"] = LR._unflat(_softmax_bwd(ar, featv, g), B)
    return out


def emulate_inputs(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0, feat=True, mutate=None, acc=torch.float64):
    assert mutate is None or mutate in MUTANTS
    ar = _Ar(False, acc, mutate)
    return _out(ar, _run_inputs(ar, sd, cfg, batch, dy_t, dy_v, drops if p > 0 else None, p, feat))


def budget_inputs(sd, cfg, batch, dy_t, dy_v, drops=None, p=0.0, feat=True):
    ar = _Ar(True)
    return _out(ar, _run_inputs(ar, sd, cfg, batch, dy_t, dy_v, drops if p > 0 else None, p, feat))


# ------------------------------------------------------------------------------------------- shared cases of the two kernels
SOFTMAX_CASES = [(1, 32), (111, 1024), (74, 2048), (5, 36)]      # below one wave's vector width; the project's widths; 36 = 4 * 9
ROW_CASES = [(1, 64), (111, 1024), (93, 768), (7, 96)]
ROW_SEED, ROW_SITE = 0x1234567, 2


def softmax_case(M, F, bf16):
    """(x, g): features (fp32 holding bf16 values when bf16) and an upstream gradient with row scales over two decades.  Row 1 carries one
    feature 30 above the others (an almost one-hot softmax), the last row is constant (M >= 3)."""
    gen = torch.Generator().manual_seed(1000 * M + F)
    x = torch.randn(M, F, generator=gen) * 2.0
    if M >= 3:
        x[1, F // 3] = x[1].max() + 30.0
        x[M - 1] = 0.75
    if bf16:
        x = x.to(torch.bfloat16).to(torch.float32)
    g = torch.randn(M, F, generator=gen) * 10.0 ** (-4.0 + 2.0 * torch.rand(M, 1, generator=gen))
    return x, g


def rows_case(M, H, p):
    """Inputs of crct_embed_input_grad: dy / saved sum as bf16 values, the statistics of the rounded sum, gamma, the location matrix
    [H, 4], the areas weight [H], text boxes with every third row empty, and the kernel's own keep mask (None at p = 0)."""
    import dropout_ref as DR
    gen = torch.Generator().manual_seed(77 * M + H)
    r = lambda *s: torch.randn(*s, generator=gen)
    dy = (r(M, H) * 10.0 ** (-5.0 + 2.0 * torch.rand(M, 1, generator=gen))).to(torch.bfloat16)
    x = (r(M, H) * 0.7 + 0.1 * r(M, 1)).to(torch.bfloat16)
    mean, rstd = row_stats(x)
    loc = torch.rand(M, 4, generator=gen)
    loc[::3] = 0.0
    keep = torch.from_numpy(DR.keep_rowmajor(ROW_SEED, ROW_SITE, M, H, p)) if p > 0 else None
    return dict(dy=dy, x=x, mean=mean, rstd=rstd, gamma=1.0 + 0.1 * r(H), w_loc=r(H, 4) * 0.05, w_areas=r(H) * 0.05, loc=loc, keep=keep, p=p)
