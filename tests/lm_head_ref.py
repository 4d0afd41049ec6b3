"""fp64 reference, emulation and error budget of the masked-LM head (crct/heads.py ``PredictionHead.loss`` / ``loss_backward``, csrc/lm_head.hip).

The head, for the rows r of ``seq`` [N, H] that carry a label (-1 = none):

    z      = LayerNorm(gelu(h W^T + b)) * gamma + beta        (eps 1e-12, erf-GELU)
    logits = z E^T + bias                                     (E = the word table [V, H])
    loss   = g * (1 / n) sum_r (logsumexp(logits_r) - logits_r[label_r])

``run(w, seq, labels, g, rnd)`` is ONE closed-form forward + backward in fp64, written out by hand (no autograd), with ``rnd`` applied
wherever the kernels store bf16: the gathered rows, the weight / table shadows, the transform's pre-activation and activation, z, the
gradient of the logits dL, dz, the LayerNorm's input gradient and the GELU's.  fp32 statistics and accumulators are taken as exact.

* ``reference(...)``: rnd = identity.  tests/test_lm_head_ref_cpu.py holds it against torch autograd of CrossEntropyLoss(ignore_index=-1).
* ``emulate(...)``: rnd = round to nearest even bf16: what the kernels compute, up to fp32 accumulation order and rounding flips.
* ``budget(...)``: per element, what the bf16 storage can cost.  Every rounding point is an independent error of at most one bf16 ulp; its
  effect on each output is measured instead of derived: DRAWS passes with STOCHASTIC rounding at every point (each value goes to one of its
  two bf16 neighbours with the probability that keeps the mean, so a draw's error per point is at most 1 ulp, against 1/2 for the
  kernels' round to nearest, and its variance at least theirs), the mean square deviation from the reference per element is the variance,
  and the budget is KSIGMA standard deviations.  A per-element variance from DRAWS = 16 samples is itself uncertain by sqrt(2 / 16) = 35 %,
  so a twentieth of the tensor's mean variance is added to each element's before the root, and FLOOR times the tensor's largest
  reference magnitude covers what fp32 accumulation adds (2^-24 relative per operation over sums of at most a few thousand terms).
  Nothing in it comes from the kernels.
"""
import math

import torch

KSIGMA = 6.0
DRAWS = 16
FLOOR = 2.0 ** -16
OUTPUTS = ("loss", "bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias", "decoder", "d_seq")


def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def stochastic_bf16(gen):
    """A rounding that sends x to the bf16 number below or above it with probabilities that keep the mean."""
    def rnd(x):
        x = x.to(torch.float32)
        bits = x.view(torch.int32)
        lo = (bits & ~0xFFFF).view(torch.float32).double()           # truncation: towards zero
        hi = ((bits & ~0xFFFF) + 0x10000).view(torch.float32).double()
        xd = x.double()
        p = torch.where(hi != lo, (xd - lo) / (hi - lo), torch.zeros_like(xd))
        up = torch.rand(x.shape, generator=gen, dtype=torch.float64) < p
        return torch.where(up, hi, lo)
    return rnd


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def run(w, seq, labels, g=1.0, rnd=None):
    """w: dict(E [V, H], bias [V], W [H, H], b [H], gamma [H], beta [H]); seq [N, H]; labels int64 [N] (-1 = no label); g: upstream scalar.
    Returns dict over OUTPUTS (fp64): loss (unscaled by g), the six parameter gradients ("decoder" = the decoder term of the word table)
    and d_seq [N, H], all of g * loss; plus per-row "loss_rows", "lse" and "rows"."""
    rnd = rnd or (lambda x: x)
    w = {k: v.detach().double() for k, v in w.items()}
    seq, labels = seq.detach().double(), labels.reshape(-1)
    rows = (labels >= 0).nonzero().flatten()
    lab = labels[rows]
    n = int(rows.numel())
    assert n > 0
    hb, W16, E16 = rnd(seq[rows]), rnd(w["W"]), rnd(w["E"])
    acc = hb @ W16.t() + w["b"]
    pre, a = rnd(acc), rnd(gelu64(acc))
    mean = a.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a - mean) ** 2).mean(1, keepdim=True) + 1e-12)
    xhat = (a - mean) * rstd
    z = rnd(xhat * w["gamma"] + w["beta"])
    logits = z @ E16.t() + w["bias"]
    lse = torch.logsumexp(logits, 1)
    loss_rows = lse - logits[torch.arange(n), lab]
    # backward of g * mean(loss_rows)
    p = torch.exp(logits - lse[:, None])
    p[torch.arange(n), lab] -= 1.0
    dL = rnd(p * (g / n))
    dz = rnd(dL @ E16)
    dxhat = dz * w["gamma"]
    dx = rnd(rstd * (dxhat - dxhat.mean(1, keepdim=True) - xhat * (dxhat * xhat).mean(1, keepdim=True)))
    dpre = rnd(dx * gelu_grad64(pre))
    d_seq = torch.zeros_like(seq)
    d_seq[rows] = dpre @ W16
    return {"loss": loss_rows.mean().reshape(1), "bias": dL.sum(0), "decoder": dL.t() @ z, "dense.weight": dpre.t() @ hb,
            "dense.bias": dpre.sum(0), "LayerNorm.weight": (dz * xhat).sum(0), "LayerNorm.bias": dz.sum(0), "d_seq": d_seq,
            "loss_rows": loss_rows, "lse": lse, "rows": rows}


def reference(w, seq, labels, g=1.0):
    return run(w, seq, labels, g)


def emulate(w, seq, labels, g=1.0):
    return run(w, seq, labels, g, bf16)


def budget(w, seq, labels, g=1.0, seed=0):
    """Per element of every output in OUTPUTS: the largest |kernel - reference| the bf16 storage accounts for (module docstring)."""
    ref = reference(w, seq, labels, g)
    gen = torch.Generator().manual_seed(seed)
    var = {k: torch.zeros_like(ref[k]) for k in OUTPUTS}
    for _ in range(DRAWS):
        out = run(w, seq, labels, g, stochastic_bf16(gen))
        for k in OUTPUTS:
            var[k] += (out[k] - ref[k]) ** 2 / DRAWS
    return {k: KSIGMA * torch.sqrt(var[k] + 0.05 * var[k].mean()) + FLOOR * ref[k].abs().max() for k in OUTPUTS}
