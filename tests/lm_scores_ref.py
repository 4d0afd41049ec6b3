"""fp64 reference, emulation and error budget of the masked-LM head's SCORES (crct/heads.py ``PredictionHead.logits`` / ``grads``, ``return_lm_scores``,
``lm_predict``), and a numpy restatement of the order ``lm_topk_rows`` sorts a row by.  Built from the pieces of tests/lm_head_ref.py.

The head on the rows ``rows`` of ``seq`` [N, H] (default: all of them):

    z      = LayerNorm(gelu(h W^T + b)) * gamma + beta        (eps 1e-12, erf-GELU)
    scores = z E^T + bias                                     (E = the word table [V, H])

and, for an upstream gradient ``G`` [R, V] on the scores scaled by ``c``, the gradients of the six tensors and of ``seq``.  ``run`` is ONE
closed-form forward + backward in fp64 (no autograd) with ``rnd`` applied wherever the kernels store bf16: the gathered rows, the weight and
table shadows, the transform's pre-activation and activation, z, the PACKED gradient dL = rnd(c G), dz, the LayerNorm's input gradient and
the GELU's.  ``reference`` / ``emulate`` / ``budget`` are built exactly as lm_head_ref builds its own: same KSIGMA, DRAWS, FLOOR, stochastic
bf16 at every storage point; nothing comes from the kernels.

The order: larger value first, then smaller column, on a monotone integer key of the fp32 bits -- -0 below +0, every NaN (any sign, any
payload) above +inf.  ``topk_ids`` is ``lexsort((index, -key))``, ``label_rank`` the number of columns in front of the label.
"""
import numpy as np
import torch

from lm_head_ref import DRAWS, FLOOR, KSIGMA, bf16, gelu64, gelu_grad64, stochastic_bf16

OUTPUTS = ("scores", "bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias", "decoder", "d_seq")


def run(w, seq, G=None, rows=None, c=1.0, rnd=None):
    """w: dict(E [V, H], bias [V], W [H, H], b [H], gamma [H], beta [H]); seq [N, H]; rows: int64 [R] (None: all N); G [R, V] or None (forward
    only).  Returns dict over OUTPUTS (fp64): scores [R, V] and, with G, the gradients of sum(c * G * scores): the six parameter gradients
    ("decoder" = the decoder term of the word table) and d_seq [N, H]."""
    rnd = rnd or (lambda x: x)
    w = {k: v.detach().double() for k, v in w.items()}
    seq = seq.detach().double()
    rows = torch.arange(seq.shape[0]) if rows is None else rows.reshape(-1).long()
    hb, W16, E16 = rnd(seq[rows]), rnd(w["W"]), rnd(w["E"])
    acc = hb @ W16.t() + w["b"]
    pre, a = rnd(acc), rnd(gelu64(acc))
    mean = a.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a - mean) ** 2).mean(1, keepdim=True) + 1e-12)
    xhat = (a - mean) * rstd
    z = rnd(xhat * w["gamma"] + w["beta"])
    out = {"scores": z @ E16.t() + w["bias"], "rows": rows}
    if G is None:
        return out
    dL = rnd(c * G.detach().double())
    dz = rnd(dL @ E16)
    dxhat = dz * w["gamma"]
    dx = rnd(rstd * (dxhat - dxhat.mean(1, keepdim=True) - xhat * (dxhat * xhat).mean(1, keepdim=True)))
    dpre = rnd(dx * gelu_grad64(pre))
    d_seq = torch.zeros_like(seq)
    d_seq[rows] = dpre @ W16
    out.update({"bias": dL.sum(0), "decoder": dL.t() @ z, "dense.weight": dpre.t() @ hb, "dense.bias": dpre.sum(0),
                "LayerNorm.weight": (dz * xhat).sum(0), "LayerNorm.bias": dz.sum(0), "d_seq": d_seq})
    return out


def reference(w, seq, G=None, rows=None, c=1.0):
    return run(w, seq, G, rows, c)


def emulate(w, seq, G=None, rows=None, c=1.0):
    return run(w, seq, G, rows, c, bf16)


def budget(w, seq, G=None, rows=None, c=1.0, seed=0):
    """Per element of every output: the largest |kernel - reference| the bf16 storage accounts for (lm_head_ref's construction)."""
    ref = reference(w, seq, G, rows, c)
    keys = [k for k in OUTPUTS if k in ref]
    gen = torch.Generator().manual_seed(seed)
    var = {k: torch.zeros_like(ref[k]) for k in keys}
    for _ in range(DRAWS):
        out = run(w, seq, G, rows, c, stochastic_bf16(gen))
        for k in keys:
            var[k] += (out[k] - ref[k]) ** 2 / DRAWS
    return {k: KSIGMA * torch.sqrt(var[k] + 0.05 * var[k].mean()) + FLOOR * ref[k].abs().max() for k in keys}


# ------------------------------------------------------------------------------------------------ the order of a row
def order_key(x):
    """int64 key of fp32 values (numpy array): larger key = earlier.  Sign bit flipped for non-negative floats, all bits for negative ones;
    every NaN gets the largest key."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0xFFFFFFFF, key).astype(np.int64)


def topk_ids(x, k):
    """[R, k] int64: the first k columns of every row of x [R, V] in the order (larger key, then smaller column)."""
    key = order_key(x)
    idx = np.arange(x.shape[1])
    return np.stack([np.lexsort((idx, -key[r]))[:k] for r in range(x.shape[0])], 0)


def label_rank(x, labels):
    """[R] int64: the number of columns of row r in front of column labels[r]."""
    key = order_key(x)
    idx = np.arange(x.shape[1])
    out = []
    for r, lab in enumerate(np.asarray(labels).reshape(-1).tolist()):
        kl = key[r, lab]
        out.append(int(((key[r] > kl) | ((key[r] == kl) & (idx < lab))).sum()))
    return np.asarray(out, dtype=np.int64)
