"""Shared helpers for the parity tests (fixture loading, weight dicts)."""
import json
import os

import numpy as np
import torch

from crct import config as C
from crct import synthetic as S
from oracle import crct_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Gradients accumulated with fp32 atomics in the embedding backward (csrc/rowops.hip row_atomic_add: position, type and colour rows): the
# order of the additions, and with it the last bits, differs from run to run.  Every other gradient is produced by deterministic kernels.
ATOMIC_GRADS = ("bert.embeddings.position_embeddings.weight", "bert.embeddings.plotqa_type_embeddings.weight",
                "bert.v_embeddings.color_emb.weight")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = C.BertConfig.from_dict(meta["cfg"])
    params = dict(meta["params"])
    params["device"] = torch.device("cpu")
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    return z, meta, cfg, params, batch


def param_shapes(cfg, params):
    """{state_dict key (no prefix): shape} for every parameter of the model (SURVEY.md 8b schema)."""
    from crct.layout import parameter_table
    table, _ = parameter_table(cfg, params)
    return {e.name: e.shape for e in table}


def seeded_weights(cfg, params, base_seed=7, requires_grad=True):
    sd = {}
    for k, shp in param_shapes(cfg, params).items():
        t = S.seeded_tensor(k, shp, base_seed)
        sd[k] = t.requires_grad_(requires_grad)
    return sd


def _engine_drop_plan(cfg, B, T, V, p_cls_hb):
    """The dropout calls of oracle_step in order, each with the engine's (site, numbering, shape): text embedding 1, image embedding 2,
    cls 3; the layers from 16 in engine.cpp's order (text layers 4 sites each, then visual layers 4 each, then connection layers 8 each),
    a self layer using site + 0 (probabilities) / + 1 (attention output) / + 2 (FFN output), a connection layer site + 0 ... + 5."""
    H, Hv = cfg.hidden_size, cfg.v_hidden_size
    L, Lv = cfg.num_hidden_layers, cfg.v_num_hidden_layers
    nh, vnh, bh = cfg.num_attention_heads, cfg.v_num_attention_heads, cfg.bi_num_attention_heads
    plan = [(1, "rows", (B, T, H)), (2, "rows", (B, V, Hv))]
    for kind, i in O.encoder_schedule(cfg):
        if kind == "t":
            s = 16 + 4 * i
            plan += [(s, "attn", (B, nh, T, T)), (s + 1, "rows", (B, T, H)), (s + 2, "rows", (B, T, H))]
        elif kind == "v":
            s = 16 + 4 * L + 4 * i
            plan += [(s, "attn", (B, vnh, V, V)), (s + 1, "rows", (B, V, Hv)), (s + 2, "rows", (B, V, Hv))]
        else:
            s = 16 + 4 * L + 4 * Lv + 8 * i
            plan += [(s, "attn", (B, bh, T, V)), (s + 1, "attn", (B, bh, V, T)), (s + 2, "rows", (B, V, Hv)), (s + 3, "rows", (B, T, H)),
                     (s + 4, "rows", (B, V, Hv)), (s + 5, "rows", (B, T, H))]
    return plan + [(3, "rows", (B, p_cls_hb))]


class _EngineDropout:
    """A stand-in for oracle._drop: call k returns x * keep / (1 - p) with the engine's mask of the k-th entry of _engine_drop_plan
    (the host Philox copy, tests/dropout_ref.py), after checking the shape that entry expects.  rewind() before every oracle pass."""

    def __init__(self, cfg, B, T, V, seed, p):
        self.plan, self.seed, self.p, self.calls, self._keep = _engine_drop_plan(cfg, B, T, V, cfg.bi_hidden_size), seed, p, [], {}

    def rewind(self):
        self.calls = []

    def __call__(self, x, prob, training):
        assert training and prob == self.p, (prob, training)
        assert len(self.calls) < len(self.plan), "more dropout calls than the engine has sites"
        site, kind, shape = self.plan[len(self.calls)]
        self.calls.append(site)
        assert tuple(x.shape) == shape, (site, kind, tuple(x.shape), shape)
        return x * self.keep_of(site, kind, shape).to(x.dtype) / (1.0 - prob)

    def keep_of(self, site, kind, shape):
        """The engine's keep mask (bool, `shape`) of dropout site `site`: kind "attn" [B, heads, Tq, Tk] or "rows" [..., width]."""
        import dropout_ref as DR
        if site not in self._keep:
            if kind == "attn":
                keep = DR.keep_attention(self.seed, site, shape[0] * shape[1], shape[2], shape[3], self.p)
            else:
                keep = DR.keep_rowmajor(self.seed, site, int(np.prod(shape[:-1])), shape[-1], self.p)
            self._keep[site] = torch.from_numpy(keep).view(shape)
        return self._keep[site]

    def check_complete(self):
        assert len(self.calls) == len(self.plan), (len(self.calls), len(self.plan))
