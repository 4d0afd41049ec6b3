"""Generate ``frozen_names.json`` by RUNNING THE REFERENCE with ``fixed_t_layer`` / ``fixed_v_layer`` (build container only).

Same import shims and model construction as ``make_golden.py``.  For each case the reference's own forward + ``loss.backward()``
runs twice on the same seeded weights and batch -- with the case's config and with both fields 0 -- and the script asserts that the
loss and every gradient that exists in the frozen run equal the unfrozen run's: freezing changes nothing above the cut.  What is
committed is only a list of names per case: the parameters whose ``.grad`` is ``None`` in the frozen run (``named_parameters()``
order, without the ``bert_pretrained.`` prefix).  No weights, no reference source.

    python tests/golden/make_golden_frozen.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G          # noqa: E402  (sets up sys.path for crct / oracle)
from crct import config as C     # noqa: E402
from crct import synthetic as S  # noqa: E402

CASES = {
    "A": dict(fixed_t_layer=1),
    "B": dict(num_hidden_layers=4, t_biattention_id=[2, 3], v_num_hidden_layers=3, v_biattention_id=[1, 2], fixed_t_layer=2,
              fixed_v_layer=1),
}


def run(vilbert, ed, cfg, params, batch):
    model = G.build_reference_model(vilbert, ed, cfg, params)
    S.seeded_fill_(model.state_dict(), base_seed=7)
    out = ed.forward(model, {k: v.clone() for k, v in batch.items()}, params)
    out[0].backward()
    grads = {k[len("bert_pretrained."):]: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    return float(out[0]), grads


def main():
    vilbert, ed = G.import_reference()
    params = C.default_params(categories=9, L1=True, device=torch.device("cpu"))
    rec = {}
    for name, over in CASES.items():
        cfg = C.tiny_config(**over)
        free = C.tiny_config(**dict(over, fixed_t_layer=0, fixed_v_layer=0))
        batch = S.make_batch(3, 9, 5, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)
        loss_f, g_f = run(vilbert, ed, cfg, params, batch)
        loss_0, g_0 = run(vilbert, ed, free, params, batch)
        assert loss_f == loss_0, (name, loss_f, loss_0)
        none = [k for k, g in g_f.items() if g is None]
        for k, g in g_f.items():
            if g is not None:
                assert g_0[k] is not None and torch.equal(g, g_0[k]), (name, k)
        only_frozen = [k for k in none if g_0[k] is not None]
        assert only_frozen, name
        print("  [%s] loss %.8f; %d parameters without gradient, %d of them because of the freeze" % (name, loss_f, len(none), len(only_frozen)))
        rec[name] = dict(config=over, grad_is_none=none)
    path = os.path.join(HERE, "frozen_names.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("  wrote", path)


if __name__ == "__main__":
    main()
