"""CPU: the yardstick of the input gradients (tests/input_grad_ref.py) is itself checked -- the clean emulator of the engine's arithmetic
stays inside the budget against fp64 at every case the GPU tests use, every mutant leaves it, and the fp64 references are what autograd
gives."""
import pytest
import torch

import input_grad_ref as IG
import layer_ref as LR
from crct import config as C
from crct import synthetic as S
from helpers import param_shapes
from test_layer_ref_cpu import P, embed_inputs

SEGMENT_CASES = [(3, 37, 31), (1, 2, 4)]


@pytest.fixture(scope="module")
def embed_model():
    """Full widths (F_v = 2048); the areas_emp Linear of the variants rides along."""
    cfg = C.vilbert_config(v_feature_size=2048)
    sd = {}
    shapes = dict(param_shapes(cfg, C.default_params()))
    shapes[LR.EV + "areas_emp.weight"], shapes[LR.EV + "areas_emp.bias"] = (cfg.v_hidden_size, 1), (cfg.v_hidden_size,)
    for k, shp in shapes.items():
        if k.startswith((LR.ET, LR.EV)):
            t = S.seeded_tensor(k, shp, 11)
            sd[k] = (t.to(torch.bfloat16) if k == LR.EV + "new_image_embeddings.weight" else t).double()
    return cfg, sd


def segment(embed_model, case, p, feat, **kw):
    cfg, sd = embed_model
    batch, dy_t, dy_v, drops = embed_inputs(cfg, case)
    # peaked rows, as class scores are: unit-variance features over 2048 classes give a softmax so flat that <s, g> is 2 % of |g|
    batch = dict(batch, image_feat=batch["image_feat"] * 4.0)
    if not feat:
        B, V = batch["image_target"].shape
        batch = dict(batch, areas=torch.rand(B, V, 1, generator=torch.Generator().manual_seed(3)))
    ref = IG.reference_inputs(sd, cfg, batch, dy_t, dy_v, drops, p, feat)
    bud = IG.budget_inputs(sd, cfg, batch, dy_t, dy_v, drops, p, feat)
    emu = IG.emulate_inputs(sd, cfg, batch, dy_t, dy_v, drops, p, feat, **kw)
    assert set(ref) == set(bud) == set(emu), sorted(set(ref) ^ set(emu))
    return {k: IG.ratio(emu[k], ref[k], bud[k]) for k in ref}, ref, batch


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", IG.SOFTMAX_CASES, ids=lambda c: "M%d_F%d" % c)
def test_clean_softmax_backward_stays_inside_the_budget_and_the_mutant_leaves_it(case, bf16):
    """Worst ratio of the fp32 emulator <= 0.9 (observed <= 0.05: the budget carries the project's fp32 slack of 2^-16); the emulator
    without the mean term sits thousands of budgets out; the rows of the fp64 reference sum to zero to fp64 rounding."""
    x, g = IG.softmax_case(*case, bf16)
    ref, bud = IG.softmax_bwd_reference(x, g), IG.softmax_bwd_budget(x, g)
    for acc in (torch.float64, torch.float32):
        r = IG.ratio(IG.softmax_bwd_emulate(x, g, acc=acc), ref, bud)
        assert float(r.max()) <= 0.9, (case, acc, float(r.max()))
    bad = IG.ratio(IG.softmax_bwd_emulate(x, g, mutate="softmax_bwd_no_mean"), ref, bud)
    print("softmax backward", case, "bf16" if bf16 else "f32", "clean %.3f, softmax_bwd_no_mean %.1f" % (float(r.max()), float(bad.max())))
    assert float(bad.max()) > 1.0
    # sum_j d_j = 0, to fp64 rounding of the terms s_j g_j it is made of (an almost one-hot row cancels far below its own |d_j|)
    scale = (torch.softmax(x.double(), -1) * g.double().abs()).sum(-1)
    assert float((ref.sum(-1).abs() / scale).max()) <= 1e-13


ROW_MUTANT_OUTPUT = {"txt_loc_mask_ignored": "d_loc", "input_grad_no_dropout_mask": "d_sum", "areas_uses_loc_weight": "d_areas"}


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", IG.ROW_CASES, ids=lambda c: "M%d_H%d" % c)
def test_clean_row_kernel_emulator_stays_inside_the_budget_and_the_mutants_leave_it(case, p):
    c = IG.rows_case(*case, p)
    args = (c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], c["keep"], p, c["w_loc"], c["loc"], c["w_areas"])
    ref, bud = IG.rows_reference(*args), IG.rows_budget(*args)
    worst = {}
    for acc in (torch.float64, torch.float32):
        emu = IG.rows_emulate(*args, acc=acc)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), float(IG.ratio(emu[k], ref[k], bud[k]).max()))
    assert all(v <= 0.9 for v in worst.values()), worst
    # rows without a box: exact zeros in the reference, hence budget 0 there
    empty = c["loc"].abs().sum(-1) == 0
    assert bool(empty.any()) and float(ref["d_loc"][empty].abs().max()) == 0.0 and float(bud["d_loc"][empty].abs().max()) == 0.0
    hits = {}
    for m, k in ROW_MUTANT_OUTPUT.items():
        if m == "input_grad_no_dropout_mask" and p == 0:
            continue
        hits[m] = float(IG.ratio(IG.rows_emulate(*args, mutate=m)[k], ref[k], bud[k]).max())
        assert hits[m] > 1.0, (m, case, p, hits[m])
    print("row kernel", case, p, "clean", {k: round(v, 3) for k, v in worst.items()}, "mutants", {k: round(v, 1) for k, v in hits.items()})


def test_row_reference_is_the_layernorm_backward_of_autograd():
    """rows_reference states the LayerNorm backward as a formula over the statistics the kernel is handed; with the exact statistics of the
    row it is autograd's gradient of dropout(LayerNorm(x))."""
    c = IG.rows_case(93, 768, 0.1)
    x = c["x"].double().clone().requires_grad_(True)
    from oracle import crct_oracle as O
    y = O.layer_norm(x, c["gamma"].double(), torch.zeros(768, dtype=torch.float64)) * LR._mask(c["keep"], 0.1)
    y.backward(c["dy"].double())
    mu = c["x"].double().mean(-1)
    rstd = 1.0 / torch.sqrt(((c["x"].double() - mu.unsqueeze(-1)) ** 2).mean(-1) + IG.EPS)
    ref = IG.rows_reference(c["dy"], c["x"], mu, rstd, c["gamma"], c["keep"], 0.1)["d_sum"]
    assert float((ref - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


@pytest.mark.parametrize("acc", [torch.float64, torch.float32], ids=["acc64", "acc32"])
@pytest.mark.parametrize("case", SEGMENT_CASES, ids=lambda c: "B%d_V%d_T%d" % c)
def test_clean_segment_emulator_stays_inside_the_budget(embed_model, case, acc):
    """Both embeddings at full widths, p = 0 and 0.1, the PlotQA form and the variants' form with areas: worst ratio <= 0.9."""
    worst = {}
    for p in (0.0, P):
        for feat in (True, False):
            r, ref, batch = segment(embed_model, case, p, feat, acc=acc)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), float(v.max()))
            empty = batch["loc"].abs().sum(-1) == 0
            assert float(ref["txt_loc"][empty].abs().max() if bool(empty.any()) else 0.0) == 0.0
            if feat:      # every row of the features' gradient sums to zero
                f = ref["image_feat"]
                assert float((f.sum(-1).abs() / f.abs().sum(-1)).max()) <= 1e-10
    print("clean input-gradient emulator, worst ratios:", case, {k: round(v, 3) for k, v in sorted(worst.items())})
    assert all(v <= 0.9 for v in worst.values()), worst


SEGMENT_MUTANT_OUTPUT = {"softmax_bwd_no_mean": ("image_feat", True), "txt_loc_mask_ignored": ("txt_loc", True),
                         "input_grad_no_dropout_mask": ("text_emb", True), "areas_uses_loc_weight": ("areas", False)}


@pytest.mark.parametrize("mutant", IG.MUTANTS)
def test_every_mutant_leaves_the_budget_of_the_segment(embed_model, mutant):
    key, feat = SEGMENT_MUTANT_OUTPUT[mutant]
    smallest, ran = float("inf"), 0
    for case in SEGMENT_CASES:
        if mutant == "txt_loc_mask_ignored" and case == (1, 2, 4):
            cfg, _ = embed_model
            if not bool((embed_inputs(cfg, case)[0]["loc"].abs().sum(-1) == 0).any()):
                continue                                   # every token of this batch has a box: the mutant cannot show
        r, _, _ = segment(embed_model, case, P, feat, mutate=mutant)
        hit = float(r[key].max())                         # (inf: a nonzero where the budget is an exact zero)
        smallest, ran = min(smallest, hit), ran + 1
        assert hit > 1.0, (mutant, case, hit)
    assert ran >= 1
    print("input-gradient mutant", mutant, "smallest worst ratio on %s: %.1f" % (key, smallest))
