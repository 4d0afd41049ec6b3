"""The per-layer yardstick (tests/layer_ref.py) proved on the CPU: one text self layer, one visual self layer and one connection layer at
the widths of config/vilbert.json, seeded weights rounded to bf16 as the shadow is, inputs with LayerNorm-like statistics, upstream
gradients at the scale the heads produce (1e-5 ... 1e-3 per element), ragged key masks."""
import os

import pytest
import torch

import dropout_ref as DR
import layer_ref as LR
from crct import config as C
from crct import synthetic as S
from helpers import param_shapes

CASES = [(3, 37, 31), (1, 2, 4), (2, 31, 31), (2, 44, 124)]          # (B, V, T)
KINDS = ("t", "v", "c")
P = 0.1
SEED = 0x5EED

torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


@pytest.fixture(scope="module")
def model():
    """cfg and {name: fp64 value} of layers t0 / v0 / c0 as the engine reads them: matrices rounded to bf16, the rest fp32."""
    cfg = C.vilbert_config(v_feature_size=2048)
    sd = {}
    for k, shp in param_shapes(cfg, C.default_params()).items():
        if k.startswith(tuple(LR.prefix_of(kind, 0) for kind in KINDS)):
            t = S.seeded_tensor(k, shp, 11)
            sd[k] = (t.to(torch.bfloat16) if len(shp) == 2 else t).double()
    return cfg, sd


def _keymask(B, L, shift):
    km = torch.ones(B, L, dtype=torch.uint8)
    for b in range(B):
        km[b, L - (L // 3 + b * max(1, L // 8) + shift) % L:] = 0 if L > 1 else 1          # ragged: rows differ by an eighth of the keys
    km[:, 0] = 1
    return km


_inputs = {}


def inputs(cfg, kind, case, scale=1.0):
    """x, dy, km, drops, dy_prev of one step; cached per (kind, case) and never modified.  dy scaled by `scale`."""
    B, V, T = case
    key = (kind, case)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * B + 10 * V + T + ord(kind))

        def act(L, H):
            x = torch.randn(B, L, H, generator=g) * (0.4 + 0.4 * torch.rand(H, generator=g)) + 0.1 * torch.randn(H, generator=g)
            return x.to(torch.bfloat16).double()

        def grad(L, H):
            row = 10.0 ** (-5.0 + 2.0 * torch.rand(B, L, 1, generator=g))
            row[-1, -1] = 1e-3          # the last row at the top of the range: a row 100 times smaller than the others is below their rounding noise
            return (torch.randn(B, L, H, generator=g) * row).to(torch.bfloat16).double()

        H, Hv = cfg.hidden_size, cfg.v_hidden_size
        km_t, km_v = _keymask(B, T, 0), _keymask(B, V, 1)
        rows = lambda site, L, W: torch.from_numpy(DR.keep_rowmajor(SEED, site, B * L, W, P)).view(B, L, W)
        attn = lambda site, h, Lq, Lk: torch.from_numpy(DR.keep_attention(SEED, site, B * h, Lq, Lk, P)).view(B, h, Lq, Lk)
        if kind == "c":
            bh = cfg.bi_num_attention_heads
            x, dy, prev, km = (act(V, Hv), act(T, H)), (grad(V, Hv), grad(T, H)), (grad(V, Hv), grad(T, H)), (km_v, km_t)
            drops = dict(attn_t=attn(64, bh, T, V), attn_v=attn(65, bh, V, T), proj_v=rows(66, V, Hv), proj_t=rows(67, T, H),
                         ffn_v=rows(68, V, Hv), ffn_t=rows(69, T, H), ffn_v_next=rows(70, V, Hv))
        else:
            L, W, h = (T, H, cfg.num_attention_heads) if kind == "t" else (V, Hv, cfg.v_num_attention_heads)
            x, dy, prev, km = act(L, W), grad(L, W), grad(L, W), (km_t if kind == "t" else km_v)
            drops = dict(attn=attn(16, h, L, L), proj=rows(17, L, W), ffn=rows(18, L, W), ffn_next=rows(19, L, W))
        _inputs[key] = (x, dy, km, drops, prev)
    x, dy, km, drops, prev = _inputs[key]
    if scale != 1.0:
        dy = tuple(d * scale for d in dy) if kind == "c" else dy * scale
        prev = tuple(d * scale for d in prev) if kind == "c" else prev * scale
    return x, dy, km, drops, prev


_refs = {}


def ref_and_budget(model, kind, case, p, r32, scale=1.0):
    key = (kind, case, p, r32, scale)
    if key not in _refs:
        cfg, sd = model
        x, dy, km, drops, _ = inputs(cfg, kind, case, scale)
        pre = LR.prefix_of(kind, 0)
        _refs[key] = (LR.reference(kind, sd, pre, cfg, x, dy, km, drops, p), LR.budget(kind, sd, pre, cfg, x, dy, km, drops, p, r32, x32=False))
    return _refs[key]


def ratios(model, kind, case, p, r32, scale=1.0, **kw):
    cfg, sd = model
    x, dy, km, drops, prev = inputs(cfg, kind, case, scale)
    ref, bud = ref_and_budget(model, kind, case, p, r32, scale)
    emu = LR.emulate(kind, sd, LR.prefix_of(kind, 0), cfg, x, dy, km, drops, p, r32, dy_prev=prev, **kw)
    assert set(emu) == set(ref) == set(bud)
    return {k: LR.ratio(emu[k], ref[k], bud[k], LR.stored_bf16(k)) for k in ref}


def test_manual_backward_equals_autograd(model):
    """The emulator's hand-written forward / backward with every rounding switched off (the budget reading carries the fp64 values) is
    the oracle block under autograd: the two agree to 2e-7 of the
    tensor's maximum on every output (the engine's 1 / (1 - p) is an fp32 constant, 3e-8 off the oracle's), which guards the emulator's and the budget's own wiring."""
    cfg, sd = model
    for kind in KINDS:
        x, dy, km, drops, _ = inputs(cfg, kind, (3, 37, 31))
        pre = LR.prefix_of(kind, 0)
        ref = LR.reference(kind, sd, pre, cfg, x, dy, km, drops, P)
        val = LR._run(LR._Ar(True), kind, sd, pre, cfg, x, dy, km, drops, P, True, False, None)
        for k, r in ref.items():
            err = float((val[k].v.reshape(r.shape) - r).abs().max())
            # the key biases' gradient is mathematically zero (softmax shift invariance): measured against the query biases' instead
            mag = float(ref[k.replace("key", "query") if k.endswith("key.bias") or k.endswith("key1.bias") or k.endswith("key2.bias") else k].abs().max())
            assert err <= 2e-7 * mag + 1e-300, (kind, k, err, mag)


def test_connection_reference_matches_the_oracle_block_directly(model):
    """A connection-layer reference at T != V is O._connection_layer in fp64 called here by hand, with the masks the right way round."""
    cfg, sd = model
    (xv, xt), (dyv, dyt), (km_v, km_t), _, _ = inputs(cfg, "c", (2, 44, 124))
    pre = LR.prefix_of("c", 0)
    ref = LR.reference("c", sd, pre, cfg, (xv, xt), (dyv, dyt), (km_v, km_t))
    from oracle import crct_oracle as O
    w = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    a, b = xv.clone().requires_grad_(True), xt.clone().requires_grad_(True)
    mv = (1.0 - km_v.double())[:, None, None, :] * -10000.0
    mt = (1.0 - km_t.double())[:, None, None, :] * -10000.0
    yv, yt = O._connection_layer(w, cfg, pre, a, mv, b, mt, False)
    ((yv * dyv).sum() + (yt * dyt).sum()).backward()
    assert torch.equal(ref["y_v"], yv.detach()) and torch.equal(ref["y_t"], yt.detach())
    assert torch.allclose(ref["gx_v"], a.grad, rtol=1e-12, atol=0) and torch.allclose(ref["gx_t"], b.grad, rtol=1e-12, atol=0)
    n = 0
    for k, v in w.items():
        if v.grad is not None:
            n += 1
            assert torch.allclose(ref[k[len(pre):]], v.grad, rtol=1e-12, atol=1e-300), k
    assert n == 32 and set(ref) == {k[len(pre):] for k, v in w.items() if v.grad is not None} | {"y_v", "y_t", "gx_v", "gx_t"}


def _group(name):
    return name if LR.stored_bf16(name) else ("d" + name.rsplit(".", 2)[-2] + "." + name.rsplit(".", 1)[-1] if "LayerNorm" in name
                                              else "d" + name.rsplit(".", 1)[-1])


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_V%d_T%d" % c)
def test_clean_emulator_stays_inside_the_budget(model, case, acc):
    """Element by element, every output of every kind, p = 0 and 0.1, both residual modes: worst ratio <= 0.9.
    Observed worst ratios over the four cases with KSIGMA = 7 (fp64 and fp32 accumulation agree to two digits: the storage roundings
    dominate): step outputs y 0.41 - 0.53, input gradients gx 0.37 - 0.55, weight gradients 0.56 - 0.69 (the maximum of up to 3 M
    elements), bias gradients 0.42 - 0.57, LayerNorm weight / bias gradients 0.39 - 0.59.  KSIGMA was chosen here: at 6 one weight
    gradient element reached 0.91 on an earlier draw of the inputs."""
    worst = {}
    for kind in KINDS:
        for p in (0.0, P):
            for r32 in (True, False):
                for k, r in ratios(model, kind, case, p, r32, acc=acc).items():
                    g = (kind, _group(k))
                    worst[g] = max(worst.get(g, 0.0), float(r.max()))
    print("clean emulator, worst ratio per (kind, output):", case, {k: round(v, 3) for k, v in sorted(worst.items())})
    bad = {k: v for k, v in worst.items() if not v <= 0.9}
    assert not bad, bad


# mutant -> (kinds, cases it can be expressed at, p, the outputs of which at least one must leave the budget)
MUTANT_CASES = {
    "ffn_residual_from_layer_input": ("tvc", CASES, 0.0, ("y", "y_v", "y_t")),
    "conn_ctx_swapped": ("c", [(2, 31, 31)], 0.0, ("y_v", "y_t")),
    "conn_wrong_keymask": ("c", [(1, 2, 4), (2, 31, 31), (2, 44, 124)], 0.0, ("y_t",)),
    "keymask_previous_row": ("tv", [(3, 37, 31), (2, 31, 31), (2, 44, 124)], 0.0, ("y",)),
    "k_wgrad_from_v_slice": ("tvc", CASES, 0.0, ("attention.self.key.weight", "biattention.key1.weight")),
    "dx_without_residual_path": ("tvc", CASES, 0.0, ("gx", "gx_v")),
    "bias_grad_drops_last_row": ("tvc", CASES, 0.0, ("intermediate.dense.bias", "v_intermediate.dense.bias", "t_intermediate.dense.bias")),
    "dropout_site_off_by_one": ("tvc", CASES, P, ("y", "y_v")),
    "stale_gradient_tile": ("tvc", CASES, 0.0, ("gx", "gx_v")),
}


@pytest.mark.parametrize("mutant", LR.MUTANTS)
def test_every_mutant_leaves_the_budget(model, mutant):
    """Each wiring error exceeds 1.0 on a named output, at every shape it can be expressed at, in both residual modes.  Smallest worst ratio on the named outputs
    over those shapes, kinds and residual modes: ffn_residual_from_layer_input 38, conn_ctx_swapped 64, conn_wrong_keymask 8.4,
    keymask_previous_row 6.2 (key masks of neighbouring rows differ by an eighth of the keys), k_wgrad_from_v_slice 553,
    dx_without_residual_path 39, bias_grad_drops_last_row 40 (the last row carries a gradient at the top of the range),
    dropout_site_off_by_one 78, stale_gradient_tile 93."""
    kinds, cases, p, names = MUTANT_CASES[mutant]
    smallest = float("inf")
    for case in cases:
        for kind in kinds:
            for r32 in (True, False):
                r = ratios(model, kind, case, p, r32, mutate=mutant)
                hit = max(float(r[k].max()) for k in names if k in r)
                smallest = min(smallest, hit)
                assert hit > 1.0, (mutant, kind, case, r32, hit)
    print("mutant", mutant, "smallest worst ratio on its named outputs: %.1f" % smallest)


def test_ratios_do_not_move_with_the_gradient_scale(model):
    """dy 2^-10: gradients, their emulated values and budgets scale by exactly 2^-10, so every ratio is bit-equal."""
    for kind in KINDS:
        a = ratios(model, kind, (3, 37, 31), P, True)
        b = ratios(model, kind, (3, 37, 31), P, True, scale=2.0 ** -10)
        for k in a:
            assert torch.equal(a[k], b[k]), (kind, k, float((a[k] - b[k]).abs().max()))


# ------------------------------------------------------------------------------------------- the two embeddings
EMBED_CASES = [(3, 37, 31), (1, 2, 4), (2, 44, 124)]


@pytest.fixture(scope="module")
def embed_model():
    cfg = C.vilbert_config(v_feature_size=2048)
    sd = {}
    for k, shp in param_shapes(cfg, C.default_params()).items():
        if k.startswith((LR.ET, LR.EV)) and "areas_emp" not in k:
            t = S.seeded_tensor(k, shp, 11)
            sd[k] = (t.to(torch.bfloat16) if k == LR.EV + "new_image_embeddings.weight" else t).double()
    return cfg, sd


def embed_inputs(cfg, case):
    B, V, T = case
    batch = S.make_batch(B, T, V, 2048, seed=100 + B, lengths=[max(4, T - 3 * b) for b in range(B)], n_vis=[max(1, V - 1 - 5 * b) for b in range(B)])
    g = torch.Generator().manual_seed(7 + B)
    grad = lambda L, H: (torch.randn(B, L, H, generator=g) * 10.0 ** (-5.0 + 2.0 * torch.rand(B, L, 1, generator=g))).to(torch.bfloat16).double()
    H, Hv = cfg.hidden_size, cfg.v_hidden_size
    drops = dict(t=torch.from_numpy(DR.keep_rowmajor(SEED, 1, B * T, H, P)).view(B, T, H),
                 v=torch.from_numpy(DR.keep_rowmajor(SEED, 2, B * V, Hv, P)).view(B, V, Hv))
    dy_t, dy_v = grad(T, H), grad(V, Hv)
    dy_t[-1, -1] = dy_t[-1, -1] * (1e-3 / dy_t[-1, -1].abs().mean() * 0.8)      # the last rows at the top of the range, as in `inputs`
    dy_v[-1, -1] = dy_v[-1, -1] * (1e-3 / dy_v[-1, -1].abs().mean() * 0.8)
    return batch, dy_t.to(torch.bfloat16).double(), dy_v.to(torch.bfloat16).double(), drops


def embed_ratios(embed_model, case, p, **kw):
    cfg, sd = embed_model
    batch, dy_t, dy_v, drops = embed_inputs(cfg, case)
    ref = LR.reference_embed(sd, cfg, batch, dy_t, dy_v, drops, p)
    bud = LR.budget_embed(sd, cfg, batch, dy_t, dy_v, drops, p)
    emu = LR.emulate_embed(sd, cfg, batch, dy_t, dy_v, drops, p, **kw)
    assert set(emu) == set(ref) == set(bud), sorted(set(emu) ^ set(ref))
    out = {}
    for k in ref:
        r = LR.ratio(emu[k], ref[k], bud[k], LR.stored_bf16(k))
        out[k] = torch.where(emu[k].reshape(ref[k].shape) == ref[k], torch.zeros_like(r), r)      # untouched table rows: exactly zero on both sides
    return out


def test_embedding_manual_backward_equals_autograd(embed_model):
    """The hand-written embeddings with every rounding off are O.embed_text / O.embed_image under autograd (2e-7 of the maximum: the fp32
    1 / (1 - p))."""
    cfg, sd = embed_model
    batch, dy_t, dy_v, drops = embed_inputs(cfg, (3, 37, 31))
    ref = LR.reference_embed(sd, cfg, batch, dy_t, dy_v, drops, P)
    val = LR._run_embed(LR._Ar(True), sd, cfg, batch, dy_t, dy_v, drops, P)
    assert set(val) == set(ref)
    for k, r in ref.items():
        err = float((val[k].v.reshape(r.shape) - r).abs().max())
        assert err <= 2e-7 * float(r.abs().max()) + 1e-300, (k, err)


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
@pytest.mark.parametrize("case", EMBED_CASES, ids=lambda c: "B%d_V%d_T%d" % c)
def test_clean_embedding_emulator_stays_inside_the_budget(embed_model, case, acc):
    """Every output of both embeddings, p = 0 and 0.1: worst ratio <= 0.9.  Observed, fp64 and fp32 accumulation alike: outputs 0.35 - 0.41,
    tables 0.27 - 0.48, location Linears 0.18 - 0.43, LayerNorm weights 0.31 - 0.55, the image Linear's matrix 0.48 - 0.61."""
    worst = {}
    for p in (0.0, P):
        for k, r in embed_ratios(embed_model, case, p, acc=acc).items():
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    print("clean embedding emulator, worst ratios:", case, {k.replace("bert.", ""): round(v, 3) for k, v in sorted(worst.items())})
    assert all(v <= 0.9 for v in worst.values()), worst


EMBED_MUTANT_OUTPUTS = {
    "embed_scatter_drops_last_row": (LR.ET + "word_embeddings.weight", LR.EV + "color_emb.weight"),
    "embed_loc_mask_ignored": (LR.ET + "txt_location_embeddings.bias",),
}


@pytest.mark.parametrize("mutant", LR.EMBED_MUTANTS)
def test_every_embedding_mutant_leaves_the_budget(embed_model, mutant):
    """Smallest worst ratio on the named outputs: embed_scatter_drops_last_row 1206, embed_loc_mask_ignored 4680."""
    smallest = float("inf")
    for case in EMBED_CASES:
        r = embed_ratios(embed_model, case, 0.0, mutate=mutant)
        hit = max(float(r[k].max()) for k in EMBED_MUTANT_OUTPUTS[mutant])
        smallest = min(smallest, hit)
        assert hit > 1.0, (mutant, case, hit)
    print("embedding mutant", mutant, "smallest worst ratio on its named outputs: %.1f" % smallest)


# ------------------------------------------------------------------------------------------- outlier channels beyond 112
def outlier_inputs(cfg):
    """Recorded inputs of one late layer: x and dy of schedule step v5 (visual self layer 5, V = 130: attention_long.hip with kept row
    statistics) of the B2_V130_T40 case of tests/test_layers_gpu.py, as the engine's taps gave them (tests/golden/layer_v5_x.npz, _dy.npz:
    bf16 bits; tests/golden/make_golden_layer_inputs.py regenerates them).  Unlike the synthetic inputs above, real hidden states have outlier channels -- a channel mean of up to 9 standard
    deviations here, 10 in the key columns -- so a key column has one sign over all keys and sum_j P_ij k_j is as large as the column."""
    import numpy as np
    from helpers import GOLDEN
    load = lambda n: torch.from_numpy(np.load(os.path.join(GOLDEN, "layer_v5_%s.npz" % n))[n].view(np.int16)).view(torch.bfloat16).double()
    km = S.make_batch(2, 40, 130, 2048, seed=102, lengths=[40, 37], n_vis=[129, 124])["image_mask"].to(torch.uint8)
    sd = {}
    for k, shp in param_shapes(cfg, C.default_params()).items():
        if k.startswith(LR.prefix_of("v", 5)):
            t = S.seeded_tensor(k, shp, 11)
            sd[k] = (t.to(torch.bfloat16) if len(shp) == 2 else t).double()
    x, dy = load("x"), load("dy")
    return sd, x, dy, km, torch.roll(dy, 1, 1)


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
def test_delta_error_reaches_dq_as_one_number(model, acc):
    """Why the budget carries the error of the attention backward's delta_i into dq coherently (layer_ref._Attn.bwd): with the outlier
    channels of real hidden states the CLEAN emulator leaves the form that adds it in quadrature over the keys (coherent_delta=False) on the query gradients, and stays
    within 0.9 of the coherent form on every output.  Four mutants are re-run there (fp64 accumulation) and still leave the budget:
    k_wgrad_from_v_slice, dx_without_residual_path, keymask_previous_row and stale_gradient_tile."""
    cfg = model[0]
    sd, x, dy, km, prev = outlier_inputs(cfg)
    pre = LR.prefix_of("v", 5)
    ref = LR.reference("v", sd, pre, cfg, x, dy, km)
    emu = LR.emulate("v", sd, pre, cfg, x, dy, km, acc=acc)
    worst = {}
    for coherent in (False, True):
        bud = LR.budget("v", sd, pre, cfg, x, dy, km, x32=False, coherent_delta=coherent)
        worst[coherent] = {k: float(LR.ratio(emu[k], ref[k], bud[k], LR.stored_bf16(k)).max()) for k in ref}
    q = "attention.self.query.weight"
    print("outlier channels, query weight gradient: quadrature form %.2f, coherent form %.2f; worst output under the coherent form %.2f" % (
        worst[False][q], worst[True][q], max(worst[True].values())))
    assert worst[False][q] > 1.0, worst[False]
    assert max(worst[True].values()) <= 0.9, worst[True]
    if acc == torch.float64:
        bud = LR.budget("v", sd, pre, cfg, x, dy, km, x32=False)
        for mutant, name in (("k_wgrad_from_v_slice", "attention.self.key.weight"), ("dx_without_residual_path", "gx"),
                             ("keymask_previous_row", "y"), ("stale_gradient_tile", "gx")):
            mu = LR.emulate("v", sd, pre, cfg, x, dy, km, mutate=mutant, dy_prev=prev)
            assert float(LR.ratio(mu[name], ref[name], bud[name], LR.stored_bf16(name)).max()) > 1.0, mutant


# ------------------------------------------------------------------------------------------- heads plus losses
HEAD_CASES = [(3, 37, 31), (1, 2, 4), (7, 3, 5)]


@pytest.fixture(scope="module")
def head_model():
    cfg = C.vilbert_config(v_feature_size=2048)
    params = C.default_params()
    sd = {}
    for k, shp in param_shapes(cfg, params).items():
        if k.rsplit(".", 1)[0] in LR.HEAD_LINEARS:
            t = S.seeded_tensor(k, shp, 11)
            sd[k] = (t.to(torch.bfloat16) if len(shp) == 2 and k not in LR.HEAD_FP32_MATRICES else t).double()
    return cfg, params, sd


def head_inputs(cfg, case):
    B, V, T = case
    batch = S.make_batch(B, T, V, 2048, seed=100 + B, needs_reg_p=0.8)
    g = torch.Generator().manual_seed(31 + B)
    act = lambda L, H: (torch.randn(B, L, H, generator=g) * (0.4 + 0.4 * torch.rand(H, generator=g)) + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16).double()
    keep = torch.from_numpy(DR.keep_rowmajor(SEED, 3, B, cfg.bi_hidden_size, P))
    return act(T, cfg.hidden_size), act(V, cfg.v_hidden_size), batch["R"], batch["next_sentence_labels"], keep


def head_ratios(head_model, case, p, **kw):
    cfg, params, sd = head_model
    xt, xv, R, labels, keep = head_inputs(cfg, case)
    ref = LR.reference_heads(sd, cfg, params, xt, xv, R, labels, keep, p)
    assert float(ref["gx_t"][:, 1:].abs().max()) == 0.0 and float(ref["gx_v"][:, 1:].abs().max()) == 0.0
    ref["gx_t"], ref["gx_v"] = ref["gx_t"][:, 0], ref["gx_v"][:, 0]
    bud = LR.budget_heads(sd, cfg, params, xt, xv, R, labels, keep, p)
    emu = LR.emulate_heads(sd, cfg, params, xt, xv, R, labels, keep, p, **kw)
    assert set(emu) == set(ref) == set(bud), sorted(set(emu) ^ set(ref))
    out = {}
    for k in ref:
        r = LR.ratio(emu[k].reshape(ref[k].shape), ref[k], bud[k].reshape(ref[k].shape), LR.stored_bf16(k))
        out[k] = torch.where(emu[k].reshape(ref[k].shape) == ref[k], torch.zeros_like(r), r)
    return out


def test_heads_manual_backward_equals_autograd(head_model):
    """The hand-written heads with every rounding off are O.heads_and_losses under autograd (2e-7 of the maximum: the fp32 1 / (1 - p))."""
    cfg, params, sd = head_model
    xt, xv, R, labels, keep = head_inputs(cfg, (3, 37, 31))
    ref = LR.reference_heads(sd, cfg, params, xt, xv, R, labels, keep, P)
    ref["gx_t"], ref["gx_v"] = ref["gx_t"][:, 0], ref["gx_v"][:, 0]
    val = LR._run_heads(LR._Ar(True), sd, cfg, params, xt, xv, R, labels, keep, P)
    assert set(val) == set(ref), sorted(set(val) ^ set(ref))
    for k, r in ref.items():
        err = float((val[k].v.reshape(r.shape) - r).abs().max())
        assert err <= 2e-7 * float(r.abs().max()) + 1e-300, (k, err, float(r.abs().max()))


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "B%d_V%d_T%d" % c)
def test_clean_heads_emulator_stays_inside_the_budget(head_model, case, acc):
    """Every output of segment 0, p = 0 and 0.1: worst ratio <= 0.9.  Observed, both accumulation types alike: logits / losses / regressed
    values 0.07 - 0.26, CLS / IMG rows 0.28 - 0.47, poolers and cls 0.12 - 0.43, pipe and fusion gradients up to 0.78."""
    worst = {}
    for p in (0.0, P):
        for k, r in head_ratios(head_model, case, p, acc=acc).items():
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    print("clean heads emulator, worst ratios:", case, {k: round(v, 3) for k, v in sorted(worst.items())})
    assert all(v <= 0.9 for v in worst.values()), worst


HEAD_MUTANT_OUTPUTS = {"heads_cat_halves_swapped": ("reg_pred", "regressor.fusion.0.weight"),
                       "heads_reg_seed_without_batch_mean": ("regressor.fusion.6.weight", "gx_t"),
                       "heads_pipe_row_overwrites_pooler_row": ("gx_t", "gx_v")}


@pytest.mark.parametrize("mutant", LR.HEAD_MUTANTS)
def test_every_heads_mutant_leaves_the_budget(head_model, mutant):
    """At the shapes with more than one batch row (1 / B cannot show at B = 1).  Smallest worst ratio on the named outputs:
    heads_cat_halves_swapped 6968, heads_reg_seed_without_batch_mean 206, heads_pipe_row_overwrites_pooler_row 52."""
    smallest = float("inf")
    for case in HEAD_CASES:
        if case[0] == 1 and mutant == "heads_reg_seed_without_batch_mean":
            continue
        r = head_ratios(head_model, case, 0.0, mutate=mutant)
        hit = max(float(r[k].max()) for k in HEAD_MUTANT_OUTPUTS[mutant])
        smallest = min(smallest, hit)
        assert hit > 1.0, (mutant, case, hit)
    print("heads mutant", mutant, "smallest worst ratio on its named outputs: %.1f" % smallest)


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
def test_clean_heads_emulator_on_recorded_hidden_states(head_model, acc):
    """The CLS / IMG rows of a real forward (tests/golden/heads_rows_B3.npz: rows 0 of the taps seq_t / seq_v of the B3_V37_T31 fp32 case of
    tests/test_layers_gpu.py, bf16 bits; tests/golden/make_golden_layer_inputs.py regenerates them).  On them several pipe and fusion units
    sit at their LeakyReLU kink, and the step between the two slopes reaches the pipe weight gradients projected through the matrices above:
    this is the case that sized how the budget enters that step (layer_ref._act_bwd).  Worst ratio 0.45; pipe weight gradients 0.37."""
    import numpy as np
    from helpers import GOLDEN
    cfg, params, sd = head_model
    z = np.load(os.path.join(GOLDEN, "heads_rows_B3.npz"))
    rows = lambda n: torch.from_numpy(z[n].view(np.int16)).view(torch.bfloat16).double()
    B, V, T = 3, 37, 31
    batch = S.make_batch(B, T, V, 2048, seed=100 + B, lengths=[max(4, T - 3 * b) for b in range(B)], n_vis=[max(1, V - 1 - 5 * b) for b in range(B)])
    args = (sd, cfg, params, rows("seq_t0")[:, None], rows("seq_v0")[:, None], batch["R"], batch["next_sentence_labels"], None, 0.0)
    ref, bud, emu = LR.reference_heads(*args), LR.budget_heads(*args), LR.emulate_heads(*args, acc=acc)
    ref["gx_t"], ref["gx_v"] = ref["gx_t"][:, 0], ref["gx_v"][:, 0]
    worst = {k: float(LR.ratio(emu[k].reshape(ref[k].shape), ref[k], bud[k].reshape(ref[k].shape), LR.stored_bf16(k)).max()) for k in ref}
    print("heads on recorded hidden states, worst ratio: %.2f" % max(worst.values()))
    assert max(worst.values()) <= 0.9, {k: v for k, v in worst.items() if v > 0.9}
