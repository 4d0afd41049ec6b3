"""Host-only yardstick for the score gradients of csrc/heads.hip (crct_head_loss_scores / crct_head_loss_variant_scores): the answer
logits and the regressed value as differentiable outputs of the head.  An fp64 restatement built from heads_ref.cls_half64 / reg_tail64
whose objective is

    g_nsp nsp + sum_b g_reg[b] rl[b] + sum_bk c Gl[b, k] logits[b, k] + sum_b c Gv[b] value[b],     value = r R[:, 3] on the needs rows, else 0

(c = grad_scale, Gl / Gv the upstream gradients of the logits and of the value), a budget per output element, an fp32 emulator of the
kernels' arithmetic in the kernels' order with the two additions and named mutants, and the inputs the CPU and GPU tests share.
tests/test_score_grad_ref_cpu.py proves the yardstick; tests/test_score_grad_kernels_gpu.py holds the kernels to it.

Budgets, by heads_ref's rule: |got - fp64| <= 2^-16 mag, mag = the sum of the absolute values of the terms that reach the element, no
absolute floor; a bf16 output gets one bf16 step more; an element nothing reaches must be exactly 0.  The new terms enter the mags as
    dlogit_k[b]   (softmax_k + [k == label]) |g_nsp| / n_valid  +  |c Gl[b, k]|
    dz[b]         |drl g_reg (1 - r^2)|  +  |c Gv[b] R[b, 3] (1 - r^2)|   (the second on the needs rows only)
and everything below them (the seeds, the four parameter gradients) is built on those two as before.
"""
import numpy as np
import torch

import heads_ref as H

F32, F64 = np.float32, np.float64
MUTANTS = ("value_unscaled", "no_tanh_slope", "grad_scale_twice", "grad_scale_missing", "upstream_dropped_on_ignored_label",
           "needs_ignored", "value_zeroed_with_target_rule", "snap_not_constant")
WHICH = ("logits", "value", "both")
BIG_Z = 3.0                                       # the row with a large |z|: 1 - r^2 = 0.0099, a hundredth of the slope at 0 (at z = 4 the
                                                  # fp32 rounding of r^2 alone, 2^-25 of 1, is a quarter of 2^-16 of 1 - r^2 = 0.0013)
SHAPES = [(B, Hb) for B in (1, 7, 300) for Hb in (64, 1032)]
# (fusion_sum, p, use_l1, kind_l1, upstream kind of heads_ref.upstream, grad_scale, labels)
COMBOS = ((0, 0.0, False, False, "default", 1.0, "some"), (1, 0.1, True, True, "loss_dev", 0.25, "some"),
          (0, 0.1, False, False, "nsp_reg_dev", 0.25, "some"), (1, 0.0, True, False, "loss_dev", 1.0, "all_ignored"))
BIG_ROW = 4                                       # an ordinary row of snap_inputs (b % 4 == 0) whose z is moved to BIG_Z


def inputs(B, Hb, seed):
    """heads_ref.snap_inputs (rows b % 4: ordinary, needs = 0, target 0 with a small r, |target| > 1; scales 40 / 47 / 49 / 100 by row)
    with row BIG_ROW moved along w_f6 until z = BIG_Z, and the targets of heads_ref.snap_targets for the fp32 r of the emulator."""
    inp = H.snap_inputs(B, Hb, seed)
    if B > BIG_ROW:
        fh, w6 = inp["fh"].float(), inp["w6"]
        row = fh[BIG_ROW].clone()
        for _ in range(8):                         # the LeakyReLU and the bf16 rounding take some of each move back
            z = float(row.to(torch.bfloat16).double() @ w6.double() + inp["b6"].double())
            row = torch.nn.functional.leaky_relu(row + (BIG_Z - z) * w6 / w6.norm() ** 2, 0.01)
        fh[BIG_ROW] = row
        inp["fh"] = fh.to(torch.bfloat16)
    return inp


def targets(inp, hc, seed):
    return H.snap_targets(inp, H.emu_tanh_r(inp), hc, seed)


def score_upstream(B, which):
    """(Gl fp32 [B, 2] or None, Gv fp32 [B] or None): ramps that cross 0, no element exactly 0."""
    Gl = (torch.linspace(-1.0, 2.0, 2 * B + 1)[:2 * B].reshape(B, 2) + 1.0 / 64).float() if which in ("logits", "both") else None
    Gv = (torch.linspace(1.5, -0.75, B + 1)[:B] + 1.0 / 128).float() if which in ("value", "both") else None
    return Gl, Gv


# ------------------------------------------------------------------------------------------- fp64
def _cls_part(inp, labels, keep, hc, g_nsp, Gl, c):
    """The classification half with the logits term in the objective: (half, the scalar to add the regression terms to, dl_mag)."""
    h = H.cls_half64(inp, labels, keep, hc)
    obj = g_nsp * h["nsp"]
    B = inp["pt"].shape[0]
    dl_mag = torch.zeros(B, 2, dtype=torch.float64)
    if labels is not None:
        valid = (labels != -1).double()[:, None]
        sm = torch.softmax(h["logits"].detach(), 1)
        onehot = torch.nn.functional.one_hot(labels.clamp_min(0), 2).double()
        dl_mag = (sm + onehot) * valid * abs(g_nsp / max(int(valid.sum()), 1))
    if Gl is not None:
        obj = obj + (c * Gl.double() * h["logits"]).sum()
        dl_mag = dl_mag + (c * Gl.double()).abs()
    return h, obj, dl_mag


def _cls_mags(inp, keep, hc, dl_mag):
    p = hc["p"]
    pt, pv = inp["pt"].double(), inp["pv"].double()
    fd = (pt + pv if hc["fusion_sum"] else pt * pv) * keep.double() / (1 - p)
    wa = inp["w_cls"].double().abs()
    df_mag = (dl_mag[:, :1] * wa[0] + dl_mag[:, 1:] * wa[1]) / (1 - p)
    return dict(d_pt=df_mag * (1 if hc["fusion_sum"] else pv), d_pv=df_mag * (1 if hc["fusion_sum"] else pt),
                d_w_cls=dl_mag.t() @ fd.abs(), d_b_cls=dl_mag.sum(0), dl=dl_mag)


def plotqa_ref64(inp, R, labels, keep, hc, *, g_nsp, g_reg, Gl=None, Gv=None, c=1.0, snap_table=None, r32=None):
    """The PlotQA head (crct_head_loss_scores), or with `snap_table` the DVQA evaluation snap from the fp32 r `r32`, where the value is a
    table constant and Gv reaches nothing.  Returns (out, grads, mags)."""
    h, obj, dl_mag = _cls_part(inp, labels, keep, hc, g_nsp, Gl, c)
    fh = inp["fh"].double().requires_grad_(True)
    w6, b6 = (inp[k].double().requires_grad_(True) for k in ("w6", "b6"))
    R64 = R.double()
    B = R.shape[0]
    zero = torch.zeros(B, dtype=torch.float64)
    z = None
    if snap_table is not None:
        sref, _, reg_mag = H.snap_ref64(inp, R, labels, keep, hc, g_nsp=g_nsp, r=r32, table=snap_table)
        out = dict(logits=h["logits"].detach(), reg=sref["reg"], stats=sref["stats"], logit_mag=h["logit_mag"])
        dz_mag = zero
    else:
        z = fh @ w6 + b6
        z.retain_grad()
        r = torch.tanh(z)
        t = H.reg_tail64(r, R, hc)
        needs, rl = t["needs"], t["rl"]
        value = torch.where(needs, r * R64[:, 3], zero)
        obj = obj + (g_reg * rl).sum()
        om = (1 - r.detach() ** 2)
        drl = torch.autograd.grad(rl.sum(), r, retain_graph=True)[0]
        dz_mag = (drl * g_reg * om).abs()
        if Gv is not None:
            obj = obj + (c * Gv.double() * value).sum()
            dz_mag = dz_mag + torch.where(needs, (c * Gv.double() * R64[:, 3] * om).abs(), zero)
        d5v = torch.where(needs, t["d5"], zero).detach()
        stats = H.head_stats(labels, h["nsp"].detach(), rl.detach(), d5v, int(needs.sum()), int(t["ok5"].sum()), int(t["okt"].sum()), h["nvalid"], B)
        reg = torch.stack([value, rl, torch.where(needs, t["l1v"], zero), r, d5v]).detach()
        zmag = inp["fh"].double().abs() @ inp["w6"].double().abs() + inp["b6"].double().abs()
        tmag = torch.where(t["target"] != 0, t["target"].abs(), torch.ones_like(zmag))
        reg_mag = torch.stack([zmag * R64[:, 3].abs(), zmag * (1 + 2 * t["l1v"].detach()), zmag, zmag, zmag / tmag]).detach()
        out = dict(logits=h["logits"].detach(), reg=reg, stats=stats, logit_mag=h["logit_mag"])
    if obj.requires_grad:
        obj.backward()
    slope = torch.where(inp["fh"].double() > 0, 1.0, 0.01)
    grads = dict(H.cls_grads(h), d_fh=H._gr(fh) * slope, d_w6=H._gr(w6), d_b6=H._gr(b6),
                 dz=z.grad if z is not None and z.grad is not None else zero)
    mags = _cls_mags(inp, keep, hc, dl_mag)
    mags.update(d_fh=dz_mag[:, None] * inp["w6"].double().abs()[None] * slope, d_w6=dz_mag @ inp["fh"].double().abs(),
                d_b6=dz_mag.sum().reshape(1), dz=dz_mag, reg=reg_mag)
    return out, grads, mags


def ce_ref64(inp, R, labels, keep, hc, *, g_nsp, g_reg, Gl, c, values):
    """The CE head with the logits term: heads_ref.ce_ref64 for the regressor (the logits do not reach it), the classification half again
    with c Gl in its objective."""
    out, grads, mags = H.ce_ref64(inp, R, labels, keep, hc, g_nsp=g_nsp, g_reg=g_reg, values=values)
    h, obj, dl_mag = _cls_part(inp, labels, keep, hc, g_nsp, Gl, c)
    if obj.requires_grad:
        obj.backward()
    grads = dict(grads, **H.cls_grads(h))
    return out, grads, dict(mags, **_cls_mags(inp, keep, hc, dl_mag))


def none_ref64(inp, R, labels, keep, hc, *, g_nsp, Gl, c):
    out, _ = H.none_ref64(inp, R, labels, keep, hc, g_nsp=g_nsp)
    h, obj, dl_mag = _cls_part(inp, labels, keep, hc, g_nsp, Gl, c)
    if obj.requires_grad:
        obj.backward()
    return out, H.cls_grads(h), _cls_mags(inp, keep, hc, dl_mag)


# ------------------------------------------------------------------------------------------- the fp32 emulator
def _np32(t):
    return t.float().numpy().astype(F32)


def emu_scores(inp, R, labels, keep, hc, grad_scale, g_loss=None, g_nsp=None, g_reg=None, Gl=None, Gv=None, prefill=None, mode="plotqa",
               mutate=None):
    """head_rows_kernel<HEAD_PLOTQA / HEAD_SNAP / HEAD_NONE> and head_reduce_kernel in fp32, in their order, from the per-row seeds on:
    dl0 / dl1 with c Gl added on every row, dz with c Gv R3 (1 - r^2) added on the needs rows, the bf16 seeds, and the parameter
    gradients as 8 row groups summed in order on top of `prefill`.  mode 'snap' takes dz = 0 whatever Gv says."""
    gn32, gr32 = H.emu_gscale(R.shape[0], grad_scale, g_loss, g_nsp, g_reg)
    cls = H.emu_cls(inp, labels, keep, hc, gn32)
    B, Hb = inp["pt"].shape
    gs = F32(grad_scale)
    c_up = {"grad_scale_twice": (gs * gs).astype(F32), "grad_scale_missing": F32(1)}.get(mutate, gs)
    dl = np.stack([cls["dl0"], cls["dl1"]], 1).astype(F32)
    if Gl is not None:
        add = np.broadcast_to(c_up, (B, 2)).astype(F32)
        g = _np32(Gl)
        if mutate == "upstream_dropped_on_ignored_label":
            g = np.where(cls["valid"][:, None], g, F32(0))
        dl = H.fma32(add, g, dl)
    Rn = R.numpy()
    needs = Rn[:, 1] == 1
    out = dict(logits=cls["logits"], dl=dl)
    pt, pv, W = _np32(inp["pt"]), _np32(inp["pv"]), _np32(inp["w_cls"])
    dsc = F32(1.0 / (1.0 - hc["p"])) if hc["p"] else F32(1)
    kp = keep.numpy()
    df = H.fma32(dl[:, 1:], W[1][None], (dl[:, :1] * W[0][None]).astype(F32))
    df = np.where(kp, (df * dsc).astype(F32), F32(0))
    gt, gv = (df, df) if hc["fusion_sum"] else ((df * pv).astype(F32), (df * pt).astype(F32))
    out["d_pt"], out["d_pv"] = H.to_bf16(np.where(pt > 0, gt, F32(0))), H.to_bf16(np.where(pv > 0, gv, F32(0)))
    dz = np.zeros(B, F32)
    if mode != "none":
        fh, w6 = _np32(inp["fh"]), _np32(inp["w6"])
        r = H.emu_tanh_r(inp)
        om = H.fma32(-r, r, np.ones(B, F32))
        with np.errstate(divide="ignore", invalid="ignore"):
            target = (Rn[:, 0] / Rn[:, 3]).astype(F32)
            diff = (r - target).astype(F32)
            l1v = np.abs(diff)
            if hc["use_l1"]:
                drl = np.sign(diff).astype(F32)
            else:
                drl = np.where(l1v < F32(0.5), (F32(2) * diff).astype(F32), np.where(diff > 0, F32(1), F32(-1)))
            dead = ~needs if hc["kind_l1"] else (~needs | (np.abs(target) > 1))
            drl = np.where(dead, F32(0), drl)
            if mode == "snap":                     # the snapped value is a constant: no loss term, and no value term either
                drl = np.zeros(B, F32)
            dz = ((drl * gr32).astype(F32) * om).astype(F32)
            if Gv is not None and (mode != "snap" or mutate == "snap_not_constant"):
                live = np.ones(B, bool) if mutate == "needs_ignored" else needs
                if mutate == "value_zeroed_with_target_rule" and not hc["kind_l1"]:
                    live = live & ~(np.abs(target) > 1)
                t = (c_up * _np32(Gv)).astype(F32)
                if mutate != "value_unscaled":
                    t = (t * Rn[:, 3]).astype(F32)
                up = t if mutate == "no_tanh_slope" else (t * om).astype(F32)
                dz = np.where(live, (dz + np.nan_to_num(up)).astype(F32), dz)
        slope = np.where(fh > 0, F32(1), F32(0.01))
        out["d_fh"] = H.to_bf16(((dz[:, None] * w6[None]).astype(F32) * slope).astype(F32))
    out["dz"] = dz
    if prefill is not None:
        fd = (pt + pv).astype(F32) if hc["fusion_sum"] else (pt * pv).astype(F32)
        fd = np.where(kp, (fd * dsc).astype(F32), F32(0))

        def reduce_rows(seed, x):                  # head_reduce_kernel: row group rg walks b = rg, rg + 8, ...; the 8 partials added in order
            part = np.zeros((8, x.shape[1]), F32)
            for b in range(B):
                part[b % 8] = H.fma32(np.broadcast_to(seed[b], x[b].shape).astype(F32), x[b], part[b % 8])
            tot = np.zeros(x.shape[1], F32)
            for k in range(8):
                tot = (tot + part[k]).astype(F32)
            return tot

        def wave_rows(v):                          # the stats wave: lane walks b = lane, lane + 64, ..., then wave_sum
            v = np.concatenate([v.astype(F32), np.zeros((-B) % 64, F32)]).reshape(-1, 64)
            acc = np.zeros(64, F32)
            for trip in v:
                acc = (acc + trip).astype(F32)
            return H.wave_sum32(acc)
        out["d_w_cls"] = (_np32(prefill["d_w_cls"]) + np.stack([reduce_rows(dl[:, 0], fd), reduce_rows(dl[:, 1], fd)])).astype(F32)
        out["d_b_cls"] = (_np32(prefill["d_b_cls"]) + np.array([wave_rows(dl[:, 0]), wave_rows(dl[:, 1])], F32)).astype(F32)
        if mode != "none":
            out["d_w6"] = (_np32(prefill["d_w6"]) + reduce_rows(dz, _np32(inp["fh"]))).astype(F32)
            out["d_b6"] = (_np32(prefill["d_b6"]) + wave_rows(dz)).astype(F32)
    return out


def prefill(B, Hb, scale=0.3):
    """The parameter-gradient prefill of test_kernels_gpu._head_launch(prefill=scale) for the PlotQA regressor (fusion.6 [256], [1])."""
    g = torch.Generator().manual_seed(B + Hb)
    return dict(d_w_cls=torch.randn(2, Hb, generator=g) * scale, d_b_cls=torch.randn(2, generator=g) * scale,
                d_w6=torch.randn(256, generator=g) * scale, d_b6=torch.randn(1, generator=g) * scale)


GRAD_KEYS = ("d_pt", "d_pv", "d_fh", "d_w_cls", "d_b_cls", "d_w6", "d_b6")
BF16_KEYS = ("d_pt", "d_pv", "d_fh")


def check_grads(got, grads, mags, pre, what, worst=None, frac=1.0, keys=GRAD_KEYS):
    """Every gradient in `keys` of `got` against fp64 at its budget; returns the messages of those that left it."""
    failed = []
    for k in keys:
        bf = k in BF16_KEYS
        ref, mag = grads[k], mags[k]
        if not bf:
            p = pre[k].double()
            ref, mag = p + ref, mag + p.abs()
        try:
            H.assert_within(got[k], ref, mag, what + ": " + k, bf16=bf, worst=worst, frac=max(frac, 0.51) if bf else frac)
        except AssertionError as e:
            failed.append(str(e))
    return failed
