"""Regenerates tests/golden/layer_v5_x.npz and layer_v5_dy.npz (needs an MI355X and the built library): the inputs of ONE schedule step
as the engine's own taps give them, for tests/test_layer_ref_cpu.py::test_delta_error_reaches_dq_as_one_number.

Case: B2_V130_T40 of tests/test_layers_gpu.py -- config/vilbert.json with v_feature_size = 2048 and every dropout probability 0,
residual_fp32 on, weights seeded_fill_ with base seed 11 (helpers.seeded_weights / S.seeded_tensor reproduce them on the host),
batch = make_batch(2, 40, 130, 2048, seed=102, lengths=[40, 37], n_vis=[129, 124]).
Step: v5 (visual self layer 5, segment 2 of 26).  x = tap "c5.v" after the training forward (the output of the step before v5 on the visual
stream); dy = tap "grad.v" after backward segment 1 (the hidden gradient segment 2 reads).  Both are stored as their bf16 bits (uint16).

Also tests/golden/heads_rows_B3.npz, for test_clean_heads_emulator_on_recorded_hidden_states: rows 0 (CLS / IMG) of the taps "seq_t" / "seq_v"
after the training forward of the B3_V37_T31 fp32 case (same model; batch = make_batch(3, 31, 37, 2048, seed=103, lengths=[31, 28, 25],
n_vis=[36, 31, 26])), as bf16 bits.

    python tests/golden/make_golden_layer_inputs.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "cqa-crct_amd"), ROOT, os.path.dirname(HERE)):
    sys.path.insert(0, p)

from crct import config as C, synthetic as S                # noqa: E402
from crct.step_adapter import forward as step_forward       # noqa: E402
from oracle import crct_oracle as O                         # noqa: E402
from test_layers_gpu import _SegmentTaps                    # noqa: E402
from test_step_gpu import build_model                       # noqa: E402


def heads_rows():
    B, V, T = 3, 37, 31
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                           v_attention_probs_dropout_prob=0.0)
    model, params = build_model(cfg, dict(C.default_params(), residual_fp32=True), weights=None, seed=11)
    model.train()
    batch = S.make_batch(B, T, V, 2048, seed=100 + B, lengths=[max(4, T - 3 * b) for b in range(B)], n_vis=[max(1, V - 1 - 5 * b) for b in range(B)])
    step_forward(model, batch, params, output_nsp_scores=True)
    torch.cuda.synchronize()
    eng = model.bert_pretrained._engine
    bits = lambda t: t.to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    np.savez_compressed(os.path.join(HERE, "heads_rows_B3.npz"), seq_t0=bits(eng.tap("seq_t", B, T, V)[:, 0]), seq_v0=bits(eng.tap("seq_v", B, T, V)[:, 0]))


def main():
    heads_rows()
    B, V, T = 2, 130, 40
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                           v_attention_probs_dropout_prob=0.0)
    model, params = build_model(cfg, dict(C.default_params(), residual_fp32=True), weights=None, seed=11)
    core = model.bert_pretrained
    model.train()
    batch = S.make_batch(B, T, V, 2048, seed=100 + B, lengths=[max(4, T - 3 * b) for b in range(B)], n_vis=[max(1, V - 1 - 5 * b) for b in range(B)])
    runner = _SegmentTaps(B, T, V)
    core._ddp = runner
    core.zero_flat_grads()
    step_forward(model, batch, params, output_nsp_scores=True)[0].backward()
    torch.cuda.synchronize()
    sched = O.encoder_schedule(cfg)
    i = sched.index(("v", 5))
    seg = len(sched) - i
    prev = "%s%d.v" % sched[max(j for j in range(i) if sched[j][0] != "t")]
    assert (prev, seg) == ("c5.v", 2), (prev, seg)
    bits = lambda t: t.to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    np.savez_compressed(os.path.join(HERE, "layer_v5_x.npz"), x=bits(core._engine.tap(prev, B, T, V)))
    np.savez_compressed(os.path.join(HERE, "layer_v5_dy.npz"), dy=bits(runner.gv[seg - 1]))


if __name__ == "__main__":
    main()
