"""fp64 reference, emulation and error budget of the masked-region head (crct/heads.py ``PredictionHead.loss`` / ``loss_backward``,
csrc/region_head.hip), in the ``run / reference / emulate / budget`` shape of tests/lm_head_ref.py, whose rounding helpers and constants
it uses.

The head, for the rows r of ``seq`` [N, Hv] whose ``image_label`` is 1 (n of them):

    z      = LayerNorm(gelu(h W^T + b)) * gamma + beta        (eps 1e-12, erf-GELU)
    logits = z D^T + d                                        (D [C, Hv], d [C]: cls.imagePredictions.decoder)
    hard targets (int64 [N], class id c):  loss_r = logsumexp(logits_r) - logits_r[c_r]
    soft targets (float [N, C], t >= 0):   loss_r = sum_j t_rj (log t_rj - log_softmax(logits_r)_j), a term with t_rj == 0 being 0
    loss   = g * (1 / max(n, 1)) sum_r loss_r

so d loss / d logits_r = (softmax(logits_r) * s_r - t_r) * g / n with s_r = sum_j t_rj (the hard form: t = one-hot, s_r = 1).

``run(w, seq, image_label, targets, g, rnd)`` is ONE closed-form forward + backward in fp64, by hand, with ``rnd`` applied wherever the
kernels store bf16: the gathered rows, the weight shadows, the transform's pre-activation and activation, z, the gradient of the logits dL,
dz, the LayerNorm's input gradient and the GELU's.  fp32 statistics, accumulators and the soft targets (read as fp32) are taken as exact.
``reference``: rnd = identity (tests/test_region_head_ref_cpu.py holds it against torch autograd); ``emulate``: round to nearest even;
``budget``: KSIGMA standard deviations of DRAWS stochastic-rounding passes per element plus FLOOR of the tensor's largest reference
magnitude -- the derivation is lm_head_ref's docstring, unchanged.  Nothing in it comes from the kernels.
"""
import torch

from lm_head_ref import DRAWS, FLOOR, KSIGMA, bf16, gelu64, gelu_grad64, stochastic_bf16

OUTPUTS = ("loss", "decoder.bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias", "decoder.weight", "d_seq")


def row_losses(logits, targets):
    """fp64 per-row loss and d loss_r / d logits_r of [n, C] logits against class ids int64 [n] or soft targets [n, C]."""
    n, C = logits.shape
    lse = torch.logsumexp(logits, 1)
    logp = logits - lse[:, None]
    if not torch.is_floating_point(targets):
        t = torch.zeros(n, C, dtype=torch.float64)
        t[torch.arange(n), targets] = 1.0
    else:
        t = targets.double()
    loss = (torch.xlogy(t, t) - torch.where(t > 0, t * logp, torch.zeros_like(t))).sum(1)
    grad = torch.exp(logp) * t.sum(1, keepdim=True) - t
    return loss, grad, lse


def run(w, seq, image_label, targets, g=1.0, rnd=None):
    """w: dict(D [C, Hv], d [C], W [Hv, Hv], b, gamma, beta [Hv]); seq [N, Hv]; image_label int64 [N] (1 = masked region); targets int64 [N]
    or float [N, C]; g: upstream scalar.  Returns dict over OUTPUTS (fp64): loss (unscaled by g), the six parameter gradients and d_seq
    [N, Hv], all of g * loss; plus per-row "loss_rows", "lse" and "rows"."""
    rnd = rnd or (lambda x: x)
    w = {k: v.detach().double() for k, v in w.items()}
    seq = seq.detach().double()
    rows = (image_label.reshape(-1) == 1).nonzero().flatten()
    n = int(rows.numel())
    assert n > 0
    tg = targets.reshape(seq.shape[0], -1)[rows] if torch.is_floating_point(targets) else targets.reshape(-1)[rows]
    hb, W16, D16 = rnd(seq[rows]), rnd(w["W"]), rnd(w["D"])
    acc = hb @ W16.t() + w["b"]
    pre, a = rnd(acc), rnd(gelu64(acc))
    mean = a.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a - mean) ** 2).mean(1, keepdim=True) + 1e-12)
    xhat = (a - mean) * rstd
    z = rnd(xhat * w["gamma"] + w["beta"])
    logits = z @ D16.t() + w["d"]
    loss_rows, grad, lse = row_losses(logits, tg)
    dL = rnd(grad * (g / n))
    dz = rnd(dL @ D16)
    dxhat = dz * w["gamma"]
    dx = rnd(rstd * (dxhat - dxhat.mean(1, keepdim=True) - xhat * (dxhat * xhat).mean(1, keepdim=True)))
    dpre = rnd(dx * gelu_grad64(pre))
    d_seq = torch.zeros_like(seq)
    d_seq[rows] = dpre @ W16
    return {"loss": (loss_rows.sum() / max(n, 1)).reshape(1), "decoder.bias": dL.sum(0), "decoder.weight": dL.t() @ z, "dense.weight": dpre.t() @ hb,
            "dense.bias": dpre.sum(0), "LayerNorm.weight": (dz * xhat).sum(0), "LayerNorm.bias": dz.sum(0), "d_seq": d_seq,
            "loss_rows": loss_rows, "lse": lse, "rows": rows}


def reference(w, seq, image_label, targets, g=1.0):
    return run(w, seq, image_label, targets, g)


def emulate(w, seq, image_label, targets, g=1.0):
    return run(w, seq, image_label, targets, g, bf16)


def budget(w, seq, image_label, targets, g=1.0, seed=0):
    """Per element of every output in OUTPUTS: the largest |kernel - reference| the bf16 storage accounts for (lm_head_ref's docstring)."""
    ref = reference(w, seq, image_label, targets, g)
    gen = torch.Generator().manual_seed(seed)
    var = {k: torch.zeros_like(ref[k]) for k in OUTPUTS}
    for _ in range(DRAWS):
        out = run(w, seq, image_label, targets, g, stochastic_bf16(gen))
        for k in OUTPUTS:
            var[k] += (out[k] - ref[k]) ** 2 / DRAWS
    return {k: KSIGMA * torch.sqrt(var[k] + 0.05 * var[k].mean()) + FLOOR * ref[k].abs().max() for k in OUTPUTS}
