"""A lazy gradient clear with both prediction heads on (-m gpu): the heads' nodes run BEFORE the engine's backward pass and open the
gradient pass themselves (``CrctModel._open_grad_pass``), so after ``zero_flat_grads(lazy=True)`` their accumulated gradients must
survive the engine's pass and the owned weight gradients must still be written, not accumulated.  Tiny config, B 3, T 9, V 5, dropout on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS                   # noqa: E402
from test_step_gpu import build_model              # noqa: E402

B, T, NV = 3, 9, 5


def test_lazy_clear_with_both_heads_matches_an_eager_clear_bit_for_bit():
    p = 0.1
    cfg = C.tiny_config(hidden_dropout_prob=p, attention_probs_dropout_prob=p, v_hidden_dropout_prob=p, v_attention_probs_dropout_prob=p)
    model, params = build_model(cfg, C.default_params(categories=9, L1=True, lm_loss_coeff=0.5, img_loss_coeff=0.5), weights=None, seed=7)
    model.train()
    core = model.bert_pretrained
    core.cls_dropout = p
    batch = S.make_batch(B, T, NV, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)
    g = torch.Generator().manual_seed(3)
    batch["mask"] = torch.where(torch.rand(B, T, generator=g) < 0.3, torch.randint(0, cfg.vocab_size, (B, T), generator=g), torch.full((B, T), -1))
    batch["mask"][0, 1], batch["mask"][2, 8] = 0, cfg.vocab_size - 1
    label = torch.full((B, NV), -1, dtype=torch.int64)
    label[:, 0] = 0
    label[0, 1] = label[1, 4] = label[2, 2] = 1
    batch["image_label"] = label
    batch["image_class"] = torch.randint(0, cfg.v_target_size, (B, NV), generator=g)

    def run(clear):
        clear()
        core._calls = 0
        out = step_forward(model, batch, params)
        assert out[1].requires_grad and out[3].requires_grad and float(out[1].detach()) > 0.0 and float(out[3].detach()) > 0.0     # both heads are on
        out[0].backward()
        torch.cuda.synchronize()
        return core.flat_grads.clone()

    eager = run(core.zero_flat_grads)                         # also the pass after which the lazy form is in force
    assert not core._wgrad_overwrite_next

    def poisoned_lazy_clear():
        core.flat_grads.fill_(float("nan"))                   # the owned weight gradients keep this until the pass writes them
        core.zero_flat_grads(lazy=True)
        assert core._wgrad_overwrite_next and core._lazy_plan is not None

    lazy = run(poisoned_lazy_clear)
    assert not core._wgrad_overwrite_next
    heads = [e for e in core.table if e.used and (e.name.startswith("cls.predictions.") or e.name.startswith("cls.imagePredictions."))]
    assert len(heads) == 11
    for e in core.table:
        if not e.used or e.name in ATOMIC_GRADS:
            continue
        a, b = eager[e.offset:e.offset + e.numel], lazy[e.offset:e.offset + e.numel]
        assert torch.isfinite(b).all(), e.name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), e.name
        if e in heads:
            assert float(b.abs().max()) > 0.0, e.name
