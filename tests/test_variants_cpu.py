"""CPU: the DVQA / FigureQA model variants' parameter schema against the reference (tests/golden/variant_*.npz, made by
tests/golden/make_golden_variants.py), the unchanged PlotQA layout, and the variants' C ABI symbols.  No GPU compute."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from crct import config as CFG
from crct import layout as LY
from crct import lib as L
from helpers import GOLDEN

CASES = ["variant_tiny_dvqa_ce", "variant_tiny_dvqa", "variant_tiny_figureqa", "variant_full_dvqa_ce", "variant_full_figureqa"]


def _meta(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("case", CASES)
def test_variant_parameter_table_matches_the_reference(case):
    z, meta = _meta(case)
    cfg = CFG.BertConfig.from_dict(meta["cfg"])
    table, total = LY.parameter_table(cfg, meta["params"])
    assert [[e.name, list(e.shape)] for e in table] == meta["named_parameters"]          # named_parameters() order and shapes
    # state_dict = the parameters + the tied LM decoder weight
    sd = {k: v for k, v in meta["state_dict"]}
    assert set(sd) == {e.name for e in table} | {"cls.predictions.decoder.weight"}
    assert all(sd[e.name] == list(e.shape) for e in table)
    # never-used tensors = the ones whose gradient is None in the reference
    unused = sorted(k[len("gradnorm."):] for k in z.files if k.startswith("gradnorm.") and float(z[k]) < 0)
    assert sorted(e.name for e in table if not e.used) == unused
    # layout invariants: 64-element alignment of every tensor, no overlaps, everything inside the flat buffer
    by_off = sorted(table, key=lambda e: e.offset)
    end = 0
    for e in by_off:
        assert e.offset >= end
        end = e.offset + e.numel
    assert end <= total


def test_variant_kinds():
    p = CFG.default_params
    assert LY.model_variant(p()) == ("plotqa", "plotqa")
    assert LY.model_variant(p(dataset="plotqa_colorless")) == ("plotqa", "plotqa")
    assert LY.model_variant(p(dataset="dvqa")) == ("dvqa", "plotqa")
    assert LY.model_variant(p(dataset="dvqa", CE_REG=True)) == ("dvqa", "ce")
    assert LY.model_variant(p(dataset="dvqa", qa_file="qa_cls.npy")) == ("dvqa", "none")
    assert LY.model_variant(p(dataset="figure_qa", binary_answers=True)) == ("figure_qa", "none")
    with pytest.raises(NotImplementedError):
        LY.model_variant(p(dataset="chartqa"))
    with pytest.raises(NotImplementedError):
        LY.model_variant(p(CE_REG=True))              # CE_REG is DVQA's regressor


# sha256 of the PlotQA tables (name, shape, offset, used, decay, language) as the parent commit builds them
PLOTQA_TABLES = [
    (lambda: (CFG.vilbert_config(), CFG.default_params()), 252666944,
     "a9346a59bf58372c7ead5900356c1352a61c05d749e1fbf1889667f7f0550719"),
    (lambda: (CFG.tiny_config(), CFG.default_params(categories=9)), 1384192,
     "938c67068971ca06918011f2f1830865622bd0dc5c79676f4a9996f1fe1ebdd7"),
    (lambda: (CFG.vilbert_config(v_feature_size=2048), CFG.default_params(dataset="plotqa_colorless")), 253715520,
     "9af5653c81f4964d75b78a83fdd548c3ce72c41889b09b78146d733743a3b747"),
]


@pytest.mark.parametrize("i", range(len(PLOTQA_TABLES)))
def test_plotqa_table_is_unchanged(i):
    make, total, digest = PLOTQA_TABLES[i]
    table, n = LY.parameter_table(*make())
    assert n == total
    assert hashlib.sha256(repr([tuple(e) for e in table]).encode()).hexdigest() == digest


def test_variant_symbols_are_exported_and_mirrored():
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = C.CDLL(L.LIB_PATH)
    for name in ("crct_embed_image_var_fwd", "crct_embed_image_var_bwd", "crct_head_loss_variant", "crct_engine_create_variant",
                 "crct_engine_set_areas"):
        assert hasattr(lib, name), name
        assert name in L.PROTOTYPES, name
    assert L.load().crct_abi_version() == 7
    assert C.sizeof(L.Variant) == 3 * 4 + 65 * 4
    assert C.sizeof(L.HeadVariantArgs) == C.sizeof(L.HeadArgs) + C.sizeof(L.Variant) + 4 + 4 + 8      # snap (+pad), ce_scratch


def test_variant_errors_before_any_gpu_work():
    lib = L.load()
    d = L.ModelDims()
    v = L.Variant()
    v.dataset, v.regressor, v.n_values = 1, 2, 3          # CE needs all 65 class values
    assert not lib.crct_engine_create_variant(C.byref(d), b"x", (C.c_int64 * 1)(0), (C.c_int64 * 1)(0), 1, 1, 1, 1, C.byref(v))
    assert b"65" in lib.crct_last_error()
    from crct.model import CrctModel
    with pytest.raises(NotImplementedError):              # fp8 is refused for the variants before the device check
        CrctModel(CFG.tiny_config(), dict(CFG.default_params(dataset="dvqa", CE_REG=True), fp8=True))
