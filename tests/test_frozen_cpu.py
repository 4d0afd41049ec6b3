"""Frozen layers (``fixed_t_layer`` / ``fixed_v_layer``, ``requires_grad_(False)``): everything that is host logic.

``tests/golden/frozen_names.json`` comes from the reference itself (tests/golden/make_golden_frozen.py): per case the names of the
parameters whose ``.grad`` is ``None`` after its own forward + backward.
"""
import json
import os
import re

import pytest
import torch

from crct import config as C
from crct import layout
from crct import lib as L
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = C.default_params(categories=9, L1=True)


def fixture():
    with open(os.path.join(GOLDEN, "frozen_names.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", ["A", "B"])
def test_the_reference_cases_validate(case):
    cfg = C.tiny_config(**fixture()[case]["config"])
    assert (cfg.fixed_t_layer, cfg.fixed_v_layer) == ((1, 0) if case == "A" else (2, 1))


def test_the_reference_asserts_hold():
    # vilbert.py:857-858: the frozen layers must lie before the first co-attention layer of their stream
    with pytest.raises(AssertionError):
        C.tiny_config(fixed_t_layer=2)          # t_biattention_id[0] == 1
    with pytest.raises(AssertionError):
        C.tiny_config(fixed_v_layer=1)          # v_biattention_id[0] == 0
    with pytest.raises(AssertionError):
        C.vilbert_config(fixed_t_layer=7)
    with pytest.raises(AssertionError):
        C.vilbert_config(fixed_v_layer=1)
    for n in range(7):                          # the shipped config: fixed_t_layer in 0..6, fixed_v_layer == 0
        assert C.vilbert_config(fixed_t_layer=n).fixed_t_layer == n


@pytest.mark.parametrize("case", ["A", "B"])
def test_layout_names_what_the_reference_leaves_without_gradient(case):
    rec = fixture()[case]
    cfg = C.tiny_config(**rec["config"])
    assert layout.frozen_names(cfg, PARAMS) == rec["grad_is_none"]
    # ... of which the freeze accounts for exactly the tensors that have a gradient with both fields 0
    free = C.tiny_config(**dict(rec["config"], fixed_t_layer=0, fixed_v_layer=0))
    never = layout.frozen_names(free, PARAMS)
    by_freeze = [n for n in rec["grad_is_none"] if n not in never]
    assert by_freeze and all(layout.is_frozen(layout.frozen_tensors(cfg), n) for n in by_freeze)
    assert layout.frozen_tensors(free) == ()
    # the tied decoder weight is the word table
    assert layout.is_frozen(layout.frozen_tensors(cfg), "cls.predictions.decoder.weight")


def test_frozen_steps_are_a_prefix_of_the_schedule_on_their_stream():
    cfg = C.tiny_config(**fixture()["B"]["config"])
    sched = layout.encoder_schedule(cfg)
    for kind, n in (("t", cfg.fixed_t_layer), ("v", cfg.fixed_v_layer)):
        mine = [s for s in sched if s[0] in (kind, "c")]
        assert mine[:n] == [(kind, i) for i in range(n)]


def test_active_blocks_cuts_the_chunk_table_on_the_host():
    """FusedAdamW's table rebuild: the blocks of segments without gradient go, segment numbers and the order stay."""
    from crct.optim import active_blocks
    blk_seg = torch.tensor([0, 0, 0, 1, 2, 2, 3, 4, 4], dtype=torch.int32)
    blk_off = torch.tensor([0, 4096, 8192, 0, 0, 4096, 0, 0, 4096], dtype=torch.int64)
    seg, off = active_blocks(blk_seg, blk_off, [True, False, True, False, True])
    assert seg.tolist() == [0, 0, 0, 2, 2, 4, 4] and off.tolist() == [0, 4096, 8192, 0, 4096, 0, 4096]
    assert seg.dtype == torch.int32 and off.dtype == torch.int64 and seg.is_contiguous() and off.is_contiguous()
    seg, off = active_blocks(blk_seg, blk_off, [True] * 5)
    assert torch.equal(seg, blk_seg) and torch.equal(off, blk_off)
    seg, off = active_blocks(blk_seg, blk_off, [False] * 5)
    assert seg.numel() == 0 and off.numel() == 0
    # the overlap plan finds a segment's blocks by bisection: a segment without blocks gets an empty range
    import bisect
    seg, _ = active_blocks(blk_seg, blk_off, [True, False, True, False, True])
    lst = seg.tolist()
    ranges = [(bisect.bisect_left(lst, s), bisect.bisect_left(lst, s + 1)) for s in range(5)]
    assert ranges == [(0, 3), (3, 3), (3, 5), (5, 5), (5, 7)]


def test_the_new_symbols_are_declared_and_mirrored():
    with open(os.path.join(ROOT, "include", "crct_hip.h")) as f:
        header = f.read()
    decl = {"crct_engine_set_trainable": r"int\s+crct_engine_set_trainable\(crct_engine_t\*,\s*const uint8_t\*\s*flags,\s*int\s+n\);",
            "crct_engine_backward_plan": r"int\s+crct_engine_backward_plan\(const crct_engine_t\*,\s*int32_t\*\s*plan,\s*int\s+cap_segments\);"}
    import ctypes as ct
    for name, pattern in decl.items():
        assert re.search(pattern, header), name
        res, args = L.PROTOTYPES[name]
        assert res is ct.c_int and len(args) == 3 and args[0] is ct.c_void_p and args[1] is ct.c_void_p and args[2] is ct.c_int
    assert re.search(r"int\s+crct_abi_version\(void\)", header)
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.crct_abi_version() == 7
        # a null engine is refused, not dereferenced
        assert lib.crct_engine_set_trainable(None, None, 0) != 0
        assert lib.crct_engine_backward_plan(None, None, 0) == -1
