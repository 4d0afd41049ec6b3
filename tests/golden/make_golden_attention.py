"""Generate tests/golden/attention_maps.npz by RUNNING THE REFERENCE (build container only): the attention maps the reference model itself
returns under ``output_all_attention_masks=True`` (vilbert.py:842-946, element 4 of the inference-branch tuple, :1661).

The reference is imported exactly as tests/golden/make_golden.py imports it (CPU, three sys.modules shims), built and filled with the
name-keyed seeded weights (seed 7) of the fixtures, put in ``eval()`` and run on the batches of two committed fixtures:
    tiny_eval           tiny config, B 3, T 7, V 5
    small_B3_V9_T130    the small long-sequence config (head sizes 32 / 48 / 32), B 3, T 130, V 9, padding in both streams
For each case every map is recorded:  <case>/t<i>  [B, heads, T, T],  <case>/v<i>  [B, v_heads, V, V],  <case>/c<i>.1  [B, bi_heads, T, V]
(attention_probs1),  <case>/c<i>.2  [B, bi_heads, V, T] (attention_probs2).  Of the 130-token text maps every 7th query row plus the last
is kept (<case>/rows); the file stays far below 1 MB.  Next to each map the yardstick  <case>/yard/<name>: the reference model's own map
under ``torch.autocast("cpu", dtype=torch.bfloat16)`` against its fp32 self, as the largest absolute deviation over the WHOLE map --
what rounding q and k to bf16 costs on this draw (the device tests/golden/make_golden.py uses for gradient norms).

    python tests/golden/make_golden_attention.py
"""
import json
import os

import numpy as np
import torch

from make_golden import HERE, build_reference_model, import_reference      # the import shims and path set-up of the other fixtures

from crct import config as C          # noqa: E402
from crct import synthetic as S       # noqa: E402
from oracle import crct_oracle as O   # noqa: E402

CASES = ("tiny_eval", "small_B3_V9_T130")


def load_fixture(name):
    z = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    return meta, C.BertConfig.from_dict(meta["cfg"]), dict(meta["params"], device=torch.device("cpu")), batch


def reference_maps(model, batch):
    T = batch["tokens"].shape[1]
    key_t = O.text_key_mask(batch["sep_indices"], batch["hist_len"], T)       # = encoder_decorator.forward :118-120
    out = model.bert_pretrained(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], sep_indices=batch["sep_indices"],
                                sep_len=batch["hist_len"] + 1, token_type_ids=batch["segments"], attention_mask=key_t,
                                image_attention_mask=batch["image_mask"], masked_lm_labels=batch["mask"], image_target=batch["image_target"],
                                gt_reg=[batch["R"], "L1"], output_all_attention_masks=True)
    maps_t, maps_v, maps_c = out[4]
    named = {}
    for i, m in enumerate(maps_t):
        named["t%d" % i] = m
    for i, m in enumerate(maps_v):
        named["v%d" % i] = m
    for i, (p1, p2) in enumerate(maps_c):
        named["c%d.1" % i], named["c%d.2" % i] = p1, p2
    return {k: v.detach().float() for k, v in named.items()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vilbert, ed = import_reference()
    rec = {}
    for case in CASES:
        meta, cfg, params, batch = load_fixture(case)
        assert meta["weight_seed"] == 7
        model = build_reference_model(vilbert, ed, cfg, params)
        S.seeded_fill_(model.state_dict(), base_seed=7)
        model.eval()
        with torch.no_grad():
            maps = reference_maps(model, batch)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                maps16 = reference_maps(model, batch)
        T = batch["tokens"].shape[1]
        assert len([k for k in maps if k[0] == "t"]) == cfg.num_hidden_layers and len([k for k in maps if k[0] == "v"]) == cfg.v_num_hidden_layers
        assert len([k for k in maps if k[0] == "c"]) == 2 * len(cfg.v_biattention_id)
        rows = sorted(set(range(0, T, 7)) | {T - 1}) if T > 112 else list(range(T))
        rec[case + "/rows"] = np.array(rows, dtype=np.int64)
        for name, m in maps.items():
            assert float((m.sum(-1) - 1).abs().max()) < 1e-5
            yard = float((maps16[name] - m).abs().max())
            rec[case + "/yard/" + name] = np.array(yard, dtype=np.float64)
            rec[case + "/" + name] = (m[:, :, rows, :] if name[0] == "t" else m).numpy()
            print("  [%s] %-5s %-18s yardstick %.3e" % (case, name, tuple(m.shape), yard))
    path = os.path.join(HERE, "attention_maps.npz")
    np.savez_compressed(path, **rec)
    print("  wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
