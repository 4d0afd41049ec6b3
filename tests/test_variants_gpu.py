"""The DVQA / FigureQA model variants on the GPU (-m gpu): the native step against the REFERENCE's outputs and gradients
(tests/golden/variant_*.npz, made by tests/golden/make_golden_variants.py), the new kernels alone against fp32 torch restatements
(CE regression head, DVQA evaluation snap, image embeddings with areas), AdamW on areas_emp without areas, and a checkpoint round
trip.  Bounds are those of the PlotQA fixtures (tests/test_step_gpu.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from crct import checkpoint as CK                  # noqa: E402
from crct import lib as L                          # noqa: E402
from crct.optim import get_optimizer               # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import load_case                      # noqa: E402
from test_step_gpu import build_model, cosine      # noqa: E402

DEV = torch.device("cuda:0")


def load_variant(name):
    """A variant fixture with its image features drawn again from meta['feat_seed'] (the files do not store them: the variant
    models never read them; tests/golden/make_golden_variants.py variant_features)."""
    z, meta, cfg, params, batch = load_case(name)
    B, V = batch["image_target"].shape
    g = torch.Generator().manual_seed(int(meta["feat_seed"]))
    batch["image_feat"] = torch.randn(B, V, cfg.v_feature_size, generator=g, dtype=torch.float32).half().float()
    return z, meta, cfg, params, batch


def sample_index(numel, n):
    """Positions of a fixture's gradient sample (make_golden_variants.py sample_index)."""
    n = min(numel, n)
    return (torch.arange(n, dtype=torch.int64) * (numel - 1)) // max(n - 1, 1)


def variant_model(meta, cfg, params):
    model, params = build_model(cfg, params, weights=None, seed=meta["weight_seed"])
    core = model.bert_pretrained
    if meta.get("ce_bias_bump"):
        c, v = meta["ce_bias_bump"]
        with torch.no_grad():
            core.regressor.ce_fusion._modules["6"].bias[c] += v
        core._invalidate_shadow()
    return model, params


def check_variant_outputs(z, out, evaluation=False, exact_choice=False):
    if evaluation:
        loss, lm, nsp, img, scores, reg = out
        assert loss is None
    else:
        loss, lm, nsp, img, scores, reg, leg = out
        ref_loss = float(z["out.loss"])
        assert abs(float(loss) - ref_loss) <= 2e-2 * abs(ref_loss), (float(loss), ref_loss)
        assert abs(float(nsp) - float(z["out.nsp_loss"][0])) <= 2e-2 * abs(float(z["out.nsp_loss"][0])) + 1e-3
    assert np.abs(scores.float().cpu().numpy() - z["out.nsp_scores"]).max() <= 3e-2
    scale = float(np.abs(z["in.R"][:, 3]).max())
    pred = reg[0].cpu().numpy()
    if exact_choice:                      # CE: the chosen class's value, the same class as the reference's
        assert np.array_equal(pred, z["out.reg_pred"]), (pred, z["out.reg_pred"])
        assert np.array_equal(reg[2].cpu().numpy(), z["out.reg_l1"]) and np.array_equal(reg[4].cpu().numpy(), z["out.reg_dist5"])
    assert np.abs(pred - z["out.reg_pred"]).max() <= 3e-2 * scale
    assert np.abs(reg[1].detach().cpu().numpy() - z["out.reg_loss"]).max() <= 3e-2
    assert np.abs(reg[2].cpu().numpy() - z["out.reg_l1"]).max() <= 3e-2
    assert isinstance(reg[3][0], int) and isinstance(reg[3][1], int)
    if exact_choice:
        assert tuple(reg[3]) == tuple(int(v) for v in z["out.reg_right"])
    assert abs(reg[3][0] - int(z["out.reg_right"][0])) <= 1 and abs(reg[3][1] - int(z["out.reg_right"][1])) <= 1


def check_gradients(z, core, full):
    bad, n = [], 0
    for k, p in core.named_parameters():
        gn = float(z["gradnorm." + k])
        if gn < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        if gn < 1e-6:
            continue                                      # key biases: mathematically zero gradient
        g = p.grad.float().reshape(-1)
        ratio = float(g.double().norm()) / gn
        if "grad." + k in z.files:
            c = cosine(g.cpu(), torch.from_numpy(z["grad." + k]).reshape(-1))
        else:
            ref = torch.from_numpy(z["gradsample." + k])
            idx = sample_index(g.numel(), ref.numel()).to(g.device)
            c = cosine(g[idx].cpu(), ref) if float(ref.norm()) > 1e-9 and ref.numel() >= 16 else 1.0
        tol_c = 0.99 if not full else (0.85 if k.startswith("regressor.") else 0.93)
        n += 1
        if c < tol_c or abs(ratio - 1) > 0.05:
            bad.append((k, c, ratio, gn))
    assert not bad, (len(bad), bad[:10])
    return n


@pytest.mark.parametrize("case", ["variant_tiny_dvqa_ce", "variant_tiny_dvqa", "variant_tiny_figureqa"])
def test_tiny_variant_step_matches_reference(case):
    z, meta, cfg, params, batch = load_variant(case)
    model, params = variant_model(meta, cfg, params)
    core = model.bert_pretrained
    assert "areas" in batch
    out = step_forward(model, batch, params)
    check_variant_outputs(z, out, exact_choice=params.get("CE_REG", False))
    out[0].backward()
    torch.cuda.synchronize()
    assert check_gradients(z, core, full=False) > 60
    assert core.bert.v_embeddings.areas_emp.weight.grad is not None


def test_tiny_dvqa_evaluation_snaps_like_the_reference():
    z, meta, cfg, params, batch = load_variant("variant_tiny_dvqa_eval")
    model, params = variant_model(meta, cfg, params)
    model.eval()
    out = step_forward(model, batch, params, evaluation=True)
    check_variant_outputs(z, out, evaluation=True)
    # every regressed value is a table value (times the row scale / scale, as the reference computes it)
    R = batch["R"]
    vals = torch.tensor(params["dvqa_floats"])
    pred = out[5][0].cpu()
    for b in range(R.shape[0]):
        if R[b, 1] == 1:
            snapped = (vals / R[b, 3]) * R[b, 3]
            assert bool((snapped == pred[b]).any()), (b, float(pred[b]))


@pytest.mark.parametrize("case", ["variant_full_dvqa_ce", "variant_full_figureqa"])
def test_full_variant_step_matches_reference(case):
    z, meta, cfg, params, batch = load_variant(case)
    model, params = variant_model(meta, cfg, params)
    core = model.bert_pretrained
    out = step_forward(model, batch, params)
    check_variant_outputs(z, out, exact_choice=params.get("CE_REG", False))
    out[0].backward()
    torch.cuda.synchronize()
    assert check_gradients(z, core, full=True) > 400


# ---------------------------------------------------------------- the kernels alone
def _head_args(B, Hb, R, labels, w6, b6, fh, ce=False, grads=True):
    g = torch.Generator(device="cpu").manual_seed(5)
    t = dict(pt=torch.relu(torch.randn(B, Hb, generator=g)).to(DEV, torch.bfloat16),
             pv=torch.relu(torch.randn(B, Hb, generator=g)).to(DEV, torch.bfloat16),
             fh=fh, w_cls=(torch.randn(2, Hb, generator=g) * 0.05).to(DEV), b_cls=torch.tensor([0.1, -0.1], device=DEV),
             w6=w6, b6=b6, R=R.to(DEV), labels=labels.to(DEV), logits=torch.zeros(B, 2, device=DEV), reg=torch.zeros(5, B, device=DEV),
             stats=torch.zeros(24, device=DEV), scratch=torch.zeros(B, 8, device=DEV),
             d_pt=torch.zeros(B, Hb, device=DEV, dtype=torch.bfloat16), d_pv=torch.zeros(B, Hb, device=DEV, dtype=torch.bfloat16),
             d_fh=torch.zeros(B, 256, device=DEV, dtype=torch.bfloat16), d_w_cls=torch.zeros(2, Hb, device=DEV),
             d_b_cls=torch.zeros(2, device=DEV), d_w6=torch.zeros_like(w6), d_b6=torch.zeros_like(b6),
             ce=torch.zeros(B, L.CE_CLASSES, device=DEV))
    a = L.HeadVariantArgs()
    h = a.h
    h.pooled_t, h.pooled_v, h.fus_h = t["pt"].data_ptr(), t["pv"].data_ptr(), t["fh"].data_ptr()
    h.w_cls, h.b_cls, h.w_f6, h.b_f6 = t["w_cls"].data_ptr(), t["b_cls"].data_ptr(), w6.data_ptr(), b6.data_ptr()
    h.R, h.labels = t["R"].data_ptr(), t["labels"].data_ptr()
    h.logits, h.reg, h.stats, h.scratch = t["logits"].data_ptr(), t["reg"].data_ptr(), t["stats"].data_ptr(), t["scratch"].data_ptr()
    if grads:
        h.d_pooled_t, h.d_pooled_v, h.d_fus_h = t["d_pt"].data_ptr(), t["d_pv"].data_ptr(), t["d_fh"].data_ptr()
        h.d_w_cls, h.d_b_cls, h.d_w_f6, h.d_b_f6 = t["d_w_cls"].data_ptr(), t["d_b_cls"].data_ptr(), t["d_w6"].data_ptr(), t["d_b6"].data_ptr()
    h.B, h.Hb, h.fusion_sum, h.use_l1, h.kind_l1 = B, Hb, 0, 1, 1
    h.tol_margin, h.nsp_coeff, h.reg_coeff, h.grad_scale = 0.01, 1.0, 0.7, 1.0
    a.ce_scratch = t["ce"].data_ptr()
    return a, t


DVQA_FLOATS = [-9.0 + i for i in range(51)] + [43.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9]


def test_ce_head_kernel_against_fp32_restatement():
    B, Hb = 12, 64
    g = torch.Generator(device="cpu").manual_seed(3)
    w6 = (torch.randn(65, 256, generator=g) * 0.1)
    b6 = torch.randn(65, generator=g) * 0.1
    chosen = torch.randint(0, 65, (B,), generator=g)
    fh = torch.randn(B, 256, generator=g) * 0.3
    fh += 25.0 * w6[chosen] / w6[chosen].norm(dim=1, keepdim=True) ** 2 * 0.1      # z[chosen] ~ +2.5: a clear top-2 margin
    fh = fh.to(torch.bfloat16)
    target = chosen.clone().float()
    target[1::3] = (chosen[1::3] + 7) % 65                                          # wrong rows
    needs = torch.ones(B)
    needs[4] = 0
    R = torch.stack([target, needs, torch.full((B,), 0.01), torch.full((B,), 100.0)], 1)
    labels = torch.randint(0, 2, (B,), generator=g)
    labels[2] = -1
    w6d, b6d = w6.to(DEV), b6.to(DEV)
    a, t = _head_args(B, Hb, R, labels, w6d, b6d, fh.to(DEV), ce=True)
    a.variant.dataset, a.variant.regressor, a.variant.n_values = 1, 2, 65
    for i, v in enumerate(DVQA_FLOATS):
        a.variant.values[i] = v
    L.check(L.load().crct_head_loss_variant(C_ref(a), L.current_stream()), "head_loss_variant")
    torch.cuda.synchronize()
    # fp32 restatement: z = ce_fusion.6(fh), p = softmax(z), CE(p, target), argmax, value lookup
    W = w6.clone().requires_grad_(True)
    bb = b6.clone().requires_grad_(True)
    fhf = fh.float().clone().requires_grad_(True)
    p = torch.softmax(fhf @ W.t() + bb, dim=1)
    tl = target.long()
    loss = F.cross_entropy(p, tl, reduction="none") * needs
    (loss.sum() * 0.7 / B).backward()
    am = p.argmax(1)
    vals = torch.tensor(DVQA_FLOATS)
    reg = t["reg"].cpu()
    assert torch.equal(reg[0], torch.where(needs == 1, vals[am], torch.zeros(B)))
    err = torch.where(needs == 1, (vals[am] - vals[tl]).abs(), torch.zeros(B))
    assert torch.equal(reg[2], err) and torch.equal(reg[4], err)
    right = int(((am == tl) & (needs == 1)).sum())
    st = t["stats"].cpu()
    assert int(st[4]) == right and int(st[5]) == right and 0 < right < B
    rel = lambda x, y: float((x - y).abs().max()) / float(y.abs().max())     # noqa: E731
    assert rel(reg[1], loss.detach()) <= 1e-5
    assert abs(float(st[2]) - float(loss.sum()) / B) <= 1e-5 * float(loss.sum()) / B
    assert rel(t["d_w6"].cpu(), W.grad) <= 1e-5 and rel(t["d_b6"].cpu(), bb.grad) <= 1e-5
    seed = fhf.grad * torch.where(fhf > 0, 1.0, 0.01)                           # gradient w.r.t. ce_fusion.4's pre-activation
    assert rel(t["d_fh"].float().cpu(), seed) <= 1e-2                            # stored as bf16


def C_ref(a):
    import ctypes
    return ctypes.byref(a)


def test_dvqa_snap_kernel_against_restatement():
    B, Hb = 16, 64
    g = torch.Generator(device="cpu").manual_seed(9)
    w6 = (torch.randn(256, generator=g) * 0.08).to(DEV)
    b6 = torch.tensor([0.05], device=DEV)
    fh = (torch.randn(B, 256, generator=g) * 0.5).to(DEV, torch.bfloat16)
    needs = torch.ones(B)
    needs[3] = 0
    R = torch.stack([torch.rand(B, generator=g) * 30, needs, torch.full((B,), 0.01), torch.full((B,), 40.0)], 1)
    labels = torch.full((B,), -1, dtype=torch.int64)
    lib = L.load()
    outs = []
    for snap in (0, 1):
        a, t = _head_args(B, Hb, R, labels, w6, b6, fh)
        a.variant.dataset, a.variant.regressor, a.variant.n_values = 1, 0, 65
        for i, v in enumerate(DVQA_FLOATS):
            a.variant.values[i] = v
        a.snap = snap
        L.check(lib.crct_head_loss_variant(C_ref(a), L.current_stream()), "head_loss_variant")
        outs.append(t)
    # without the snap the variant entry point is crct_head_loss itself, bit for bit
    a0, t0 = _head_args(B, Hb, R, labels, w6, b6, fh)
    L.check(lib.crct_head_loss(C_ref(a0.h), L.current_stream()), "head_loss")
    torch.cuda.synchronize()
    for k in ("reg", "stats", "logits", "d_fh", "d_w6", "d_b6"):
        assert torch.equal(outs[0][k], t0[k]), k
    t = outs[1]
    reg = t["reg"].cpu()
    raw = reg[3]                                          # tanh output before the snap
    x = raw * R[:, 3]
    vals = torch.tensor(DVQA_FLOATS)
    idx = (vals[None, :] - x[:, None]).abs().argmin(1)    # first minimum, fp32 distances
    r = vals[idx] / R[:, 3]
    target = R[:, 0] / R[:, 3]
    l1 = (r - target).abs()
    assert torch.equal(reg[0], torch.where(needs == 1, r * R[:, 3], torch.zeros(B)))
    assert torch.equal(reg[2], torch.where(needs == 1, l1, torch.zeros(B)))
    assert torch.equal(reg[1], torch.where(needs == 1, l1, torch.zeros(B)))          # L1 (evaluation kind)
    d5 = torch.where(target == 0, torch.ones(B), l1 / target.abs())
    ok5 = ((d5 <= 0.05) & (needs == 1)).sum()
    okt = ((l1 <= 0.01) & (needs == 1)).sum()
    st = t["stats"].cpu()
    assert int(st[4]) == int(ok5) and int(st[5]) == int(okt)
    assert float(t["d_fh"].float().abs().max()) == 0.0 and float(t["d_w6"].abs().max()) == 0.0     # the snapped value is a constant


@pytest.mark.parametrize("H", [96, 1024])
def test_areas_embedding_against_autograd(H):
    M, n_color = 75, 11
    g = torch.Generator(device="cpu").manual_seed(H)
    loc = torch.rand(M, 4, generator=g)
    target = torch.randint(0, n_color, (M,), generator=g)
    areas = torch.rand(M, generator=g)
    wl, bl = torch.randn(H, 4, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    color = torch.randn(n_color, H, generator=g) * 0.1
    wa, ba = torch.randn(H, 1, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    gam, bet = 1 + torch.randn(H, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    dy = torch.randn(M, H, generator=g).to(torch.bfloat16)
    d = {k: v.to(DEV).contiguous() for k, v in dict(loc=loc, target=target, areas=areas, wl=wl, bl=bl, color=color, wa=wa, ba=ba,
                                                  gam=gam, bet=bet, dy=dy).items()}
    lib = L.load()
    nblk = lib.crct_layernorm_bwd_blocks(M)
    s = L.current_stream()

    def run(with_areas):
        o = dict(sum=torch.empty(M, H, device=DEV, dtype=torch.bfloat16), y=torch.empty(M, H, device=DEV, dtype=torch.bfloat16),
                 mean=torch.empty(M, device=DEV), rstd=torch.empty(M, device=DEV), d_color=torch.zeros(n_color, H, device=DEV),
                 d_wl=torch.zeros(H, 4, device=DEV), d_bl=torch.zeros(H, device=DEV), d_wa=torch.zeros(H, 1, device=DEV),
                 d_ba=torch.zeros(H, device=DEV), d_g=torch.zeros(H, device=DEV), d_b=torch.zeros(H, device=DEV),
                 part=torch.empty(8 * 4 * nblk * H, device=DEV), rows=torch.empty(M, H, device=DEV),
                 idx=torch.empty(M, device=DEV, dtype=torch.int32))
        ar = d["areas"].data_ptr() if with_areas else None
        L.check(lib.crct_embed_image_var_fwd(d["loc"].data_ptr(), d["target"].data_ptr(), ar, d["wl"].data_ptr(), d["bl"].data_ptr(),
                                             d["color"].data_ptr(), d["wa"].data_ptr(), d["ba"].data_ptr(), d["gam"].data_ptr(),
                                             d["bet"].data_ptr(), o["sum"].data_ptr(), o["y"].data_ptr(), o["mean"].data_ptr(),
                                             o["rstd"].data_ptr(), M, H, 1e-12, 0, 1.0, 0, 0, s), "embed_image_var_fwd")
        L.check(lib.crct_embed_image_var_bwd(d["dy"].data_ptr(), o["sum"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(),
                                             d["loc"].data_ptr(), d["target"].data_ptr(), ar, d["gam"].data_ptr(), o["d_color"].data_ptr(),
                                             o["d_wl"].data_ptr(), o["d_bl"].data_ptr(), o["d_wa"].data_ptr(), o["d_ba"].data_ptr(),
                                             o["d_g"].data_ptr(), o["d_b"].data_ptr(), o["part"].data_ptr(), M, H, 0, 1.0, 0, 0,
                                             o["rows"].data_ptr(), o["idx"].data_ptr(), n_color, s), "embed_image_var_bwd")
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items() if k not in ("part", "rows", "idx")}

    o = run(True)
    # restatement: vilbert.py:1478-1489 (sum in fp32, saved as bf16), LayerNorm over the saved row, autograd for the gradients
    ref_sum = loc @ wl.t() + bl + color[target] + (areas[:, None] * wa[:, 0] + ba)
    assert float((o["sum"].float() - ref_sum).abs().max()) <= 1e-2 * float(ref_sum.abs().max())
    x = o["sum"].float().clone().requires_grad_(True)
    gg, bt = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    y = F.layer_norm(x, (H,), gg, bt, eps=1e-12)
    assert float((o["y"].float() - y.detach()).abs().max()) <= 2e-2
    y.backward(dy.float())
    ds = x.grad
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())     # noqa: E731
    assert rel(o["d_wa"][:, 0], (ds * areas[:, None]).sum(0)) <= 1e-4
    assert rel(o["d_ba"], ds.sum(0)) <= 1e-4 and rel(o["d_bl"], ds.sum(0)) <= 1e-4
    assert rel(o["d_wl"], ds.t() @ loc) <= 1e-4
    assert rel(o["d_color"], torch.zeros(n_color, H).index_add_(0, target, ds)) <= 1e-4
    assert rel(o["d_g"], gg.grad) <= 1e-4 and rel(o["d_b"], bt.grad) <= 1e-4
    # fixed summation order: bit-identical on a second run
    o2 = run(True)
    for k in o:
        assert torch.equal(o[k], o2[k]), k
    # without areas: no areas term, its gradients untouched
    o3 = run(False)
    assert float(o3["d_wa"].abs().max()) == 0.0 and float(o3["d_ba"].abs().max()) == 0.0
    ref3 = loc @ wl.t() + bl + color[target]
    assert float((o3["sum"].float() - ref3).abs().max()) <= 1e-2 * float(ref3.abs().max())


@pytest.mark.parametrize("case", ["tiny_L1", "variant_tiny_dvqa_ce", "variant_tiny_dvqa", "variant_tiny_figureqa"])
def test_mask_prob_img_is_refused_in_training(case):
    """params['mask_prob_img'] > 0 zeroes whole visual elements in the reference's training forward (vilbert.py:1491-1493); this step
    has no such masking, so a training forward with it is an error that names the option, on every dataset variant.  Evaluation
    forwards (where the reference does not mask) and the value 0 are unaffected."""
    if case.startswith("variant"):
        z, meta, cfg, params, batch = load_variant(case)
        model, params = variant_model(meta, cfg, params)
    else:
        z, meta, cfg, params, batch = load_case(case)
        model, params = build_model(cfg, params, weights=z)
    core = model.bert_pretrained
    assert core.params is params
    model.eval()
    ev = step_forward(model, batch, params, evaluation=True)[4].clone()
    model.train()
    params["mask_prob_img"] = 0.15
    with pytest.raises(RuntimeError, match="mask_prob_img"):
        step_forward(model, batch, params)
    model.eval()
    assert torch.equal(step_forward(model, batch, params, evaluation=True)[4], ev)
    model.train()
    params["mask_prob_img"] = 0.0
    out = step_forward(model, batch, params)
    assert torch.isfinite(out[0])


# ---------------------------------------------------------------- optimizer / checkpoint
def test_adamw_leaves_areas_emp_alone_without_areas():
    z, meta, cfg, params, batch = load_variant("variant_tiny_dvqa_ce")
    model, params = variant_model(meta, cfg, params)
    core = model.bert_pretrained
    opt = get_optimizer(params, model)
    emb = core.bert.v_embeddings
    areas_w0, areas_b0 = emb.areas_emp.weight.detach().clone(), emb.areas_emp.bias.detach().clone()
    img_w0 = emb.new_image_embeddings.weight.detach().clone()
    loc_w0 = emb.new_loc_emb.weight.detach().clone()
    plain = {k: v for k, v in batch.items() if k != "areas"}
    for _ in range(3):
        step_forward(model, plain, params)[0].backward()
        assert emb.areas_emp.weight.grad is None                     # as torch leaves a parameter no pass reached
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    assert torch.equal(emb.areas_emp.weight.detach(), areas_w0) and torch.equal(emb.areas_emp.bias.detach(), areas_b0)
    for e in core.optional_entries:
        assert float(opt._m[e.offset:e.offset + e.numel].abs().max()) == 0.0
        assert float(opt._v[e.offset:e.offset + e.numel].abs().max()) == 0.0
    assert not torch.equal(emb.new_loc_emb.weight.detach(), loc_w0)       # everything else trains
    assert torch.equal(emb.new_image_embeddings.weight.detach(), img_w0)
    # with areas the tensor trains; the image-feature Linear never does
    step_forward(model, batch, params)[0].backward()
    assert emb.areas_emp.weight.grad is not None and float(emb.areas_emp.weight.grad.abs().max()) > 0
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    assert not torch.equal(emb.areas_emp.weight.detach(), areas_w0)
    assert torch.equal(emb.new_image_embeddings.weight.detach(), img_w0)
    assert torch.equal(core.flat_shadow[core._entries["bert.v_embeddings.areas_emp.weight"].offset:][:4].float(),
                       emb.areas_emp.weight.detach().reshape(-1)[:4].to(torch.bfloat16).float())


def test_new_image_embeddings_unchanged_after_three_adamw_steps():
    z, meta, cfg, params, batch = load_variant("variant_tiny_figureqa")
    model, params = variant_model(meta, cfg, params)
    emb = model.bert_pretrained.bert.v_embeddings
    opt = get_optimizer(params, model)
    w0, b0, sep0 = (emb.new_image_embeddings.weight.detach().clone(), emb.new_image_embeddings.bias.detach().clone(),
                    emb.sep_emb.weight.detach().clone())
    for _ in range(3):
        step_forward(model, batch, params)[0].backward()
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    assert torch.equal(emb.new_image_embeddings.weight.detach(), w0) and torch.equal(emb.new_image_embeddings.bias.detach(), b0)
    assert torch.equal(emb.sep_emb.weight.detach(), sep0)
    assert emb.new_image_embeddings.weight.grad is None and emb.sep_emb.weight.grad is None


def test_checkpoint_round_trip_dvqa_ce(tmp_path):
    from crct.optim import WarmupLinearScheduleNonZero
    z, meta, cfg, params, batch = load_variant("variant_tiny_dvqa_ce")
    model, params = variant_model(meta, cfg, params)
    opt = get_optimizer(params, model)
    sched = WarmupLinearScheduleNonZero(opt, warmup_steps=4, t_total=10, min_lr=1.3e-5)
    step_forward(model, batch, params)[0].backward()
    opt.step()
    opt.zero_grad()
    sched.step()
    path = CK.save_checkpoint(str(tmp_path), model, opt, sched, epoch=0, step_iter_id=0)
    back = torch.load(path, map_location="cpu", weights_only=False)
    keys = [k[len("bert_pretrained."):] for k in back["model_state_dict"]]
    assert [k for k, _ in meta["state_dict"]] == keys
    assert any(k.startswith("regressor.ce_fusion.6.") for k in keys) and not any(".fusion." in k for k in keys)
    model2, _ = variant_model(meta, cfg, params)
    assert CK.load_model_weights(model2, path) == len(keys)
    for k, v in model.state_dict().items():
        assert torch.equal(v, model2.state_dict()[k]), k
    model.eval()
    model2.eval()
    o1 = step_forward(model, batch, params, evaluation=True)
    o2 = step_forward(model2, batch, params, evaluation=True)
    assert torch.equal(o1[4], o2[4]) and torch.equal(o1[5][0], o2[5][0])
