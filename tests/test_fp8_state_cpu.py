"""The host logic of the fp8 step (crct/fp8.py) without a GPU: the optimizer-segment -> shadow-slot / transposed-band map, the tile
table of the transposed copy, the forward and backward protocol decisions over all of their inputs, and the window counter of a scale
family.  Every expected value is derived by hand from the rule it follows from, never by calling the function under test."""
import inspect
import itertools

import pytest

from crct import fp8 as F8

# Three shadowed weights in the engine's model order, which is NOT the order of their offsets: (offset, numel), stored [out][in]
#   slot 0: (16384, 8192), in 64 -> out 128      slot 1: (0, 12288), in 64 -> out 192 (a fused QKV weight)      slot 2: (32768, 4096), in 32 -> out 128
WEIGHTS = [(16384, 8192), (0, 12288), (32768, 4096)]
W_IN = [64, 64, 32]
# the optimizer's segments are parameter tensors: Q, K, V of the fused weight, a bias, W0, a bias, W2
Q, K, V, B0, W0, B1, W2 = (0, 4096), (4096, 4096), (8192, 4096), (12288, 192), (16384, 8192), (24576, 128), (32768, 4096)
SEGS = [Q, K, V, B0, W0, B1, W2]


def test_segment_shadow_map_on_a_fused_qkv_layout():
    slots, t_in, t_base, t_ld, fused = F8.segment_shadow_map(WEIGHTS, W_IN, SEGS, True)
    # slot = the weight whose [offset, offset + numel) holds the segment: Q, K, V lie in [0, 12288) = slot 1; W0 = slot 0; W2 = slot 2;
    # the biases start where a weight ends (12288 = 0 + 12288, 24576 = 16384 + 8192) and lie in none
    assert slots == [1, 1, 1, -1, 0, -1, 2]
    # a band of whole rows in whole 64 x 64 tiles: in % 64 == 0, the segment starts at a row (offset % in == 0) that is a multiple of 16
    # and holds a multiple of 64 rows (numel % (64 * in) == 0).  Q / K / V: in 64, rows 0 / 64 / 128, 4096 = 64 * 64 elements: yes.
    # W0: in 64, row 0, 8192 = 2 * 64 * 64: yes.  W2: in 32 is no multiple of 64: no.  Biases: in no weight.
    assert t_in == [64, 64, 64, 0, 64, 0, 0]
    # first byte of the band in the transposed copy [in][out]: the weight's offset + the band's first row = 0 + 0, 0 + 4096 / 64,
    # 0 + 8192 / 64; 16384 + 0
    assert t_base == [0, 64, 128, 0, 16384, 0, 0]
    # leading dimension of the transposed copy = out of the whole weight: 12288 / 64 = 192, 8192 / 64 = 128
    assert t_ld == [192, 192, 192, 0, 128, 0, 0]
    # the bands cover slot 0 (8192 of 8192) and slot 1 (3 * 4096 of 12288) but nothing of slot 2 (in % 64 != 0): the separate launch stays
    assert fused is False


def test_segment_shadow_map_is_fused_when_every_weight_is_covered_by_bands():
    slots, t_in, t_base, t_ld, fused = F8.segment_shadow_map(WEIGHTS[:2], W_IN[:2], SEGS[:6], True)
    assert slots == [1, 1, 1, -1, 0, -1] and t_in == [64, 64, 64, 0, 64, 0]          # as above, without slot 2 / W2
    assert fused is True                                                            # 8192 of 8192 and 12288 of 12288


def test_segment_shadow_map_without_a_transposed_copy():
    slots, t_in, t_base, t_ld, fused = F8.segment_shadow_map(WEIGHTS, W_IN, SEGS, False)
    assert slots == [1, 1, 1, -1, 0, -1, 2]                                         # the shadow itself is maintained all the same
    assert t_in == [0] * 7 and t_base == [0] * 7 and t_ld == [0] * 7 and fused is False


def test_segment_shadow_map_refuses_a_band_that_starts_off_a_16_row_boundary():
    # one weight [72][64] split into rows 0-7 (512 elements: no multiple of 64 rows) and rows 8-71 (64 rows = 4096 elements, in 64, starts
    # at a row -- but row 8 is no multiple of 16): neither is a band
    slots, t_in, t_base, t_ld, fused = F8.segment_shadow_map([(0, 4608)], [64], [(0, 512), (512, 4096)], True)
    assert slots == [0, 0] and t_in == [0, 0] and t_base == [0, 0] and t_ld == [0, 0] and fused is False


def test_segment_shadow_map_refuses_segments_that_miss_a_weight():
    with pytest.raises(RuntimeError, match="1 of the model's 3 fp8-shadowed weights are not covered by optimizer segments"):
        F8.segment_shadow_map(WEIGHTS, W_IN, [s for s in SEGS if s is not W0], True)


def test_tile_table():
    # 64 x 64 tiles of [out][in]: slot 0 [128][64] = 2 x 1, slot 1 [192][64] = 3 x 1, slot 2 [128][32] = 2 x 1 (a ragged tile counts)
    assert F8.tile_table(WEIGHTS, W_IN) == ([0, 2, 5], 7)


# ------------------------------------------------------------------------------------------- protocol decisions
# CrctModel.forward, as it stood before crct/fp8.py: neither fp8 forward nor fp8 weight gradients = data gradients only -- the state
# goes along only where a backward pass follows (train_grad), no dry pass, no scale update, step['fp8_mode'] stays unset (= 1),
# step['fp8_backward_only'] set.  Inputs: (fp8_forward, fp8_wgrad, train_grad); the other three do not matter.
BACKWARD_ONLY = {(0, 0, 0): (False, False, False, 1, True),
                 (0, 0, 1): (True, False, False, 1, True)}
# Otherwise the state always goes along; (training, calibrated, scaled) -> (dry pass = not calibrated, update = training or not scaled)
DRY_AND_UPDATE = {(0, 0, 0): (True, True), (0, 0, 1): (True, False), (0, 1, 0): (False, True), (0, 1, 1): (False, False),
                  (1, 0, 0): (True, True), (1, 0, 1): (True, True), (1, 1, 0): (False, True), (1, 1, 1): (False, True)}
# ... and (fp8_forward, fp8_wgrad) -> fp8_mode: 2 (bf16 forward GEMMs, copies and maxima still written) exactly when fp8_forward is off
FP8_MODE = {(1, 0): 1, (1, 1): 1, (0, 1): 2}
# CrctModel._run_backward: (bwd_calibrated, g_scales_fresh) -> (mode: 2 on the first pass, 1 after; update first: mode 1 with stale scales)
BACKWARD = {(0, 0): (2, False), (0, 1): (2, False), (1, 0): (1, True), (1, 1): (1, False)}

MUTANTS = {"or_to_and": ("forward_plan", "training or not scaled", "training and not scaled"),
           "scaled_term_dropped": ("forward_plan", "training or not scaled", "training"),
           "modes_swapped": ("backward_plan", "1 if bwd_calibrated else 2", "2 if bwd_calibrated else 1")}


def _plans(mutate=None):
    """(forward_plan, backward_plan) of crct/fp8.py; ``mutate``: one of MUTANTS, applied to the function's own source text."""
    fns = dict(forward_plan=F8.forward_plan, backward_plan=F8.backward_plan)
    if mutate is not None:
        name, old, new = MUTANTS[mutate]
        src = inspect.getsource(fns[name])
        assert src.count(old) == 1, (mutate, "the mutated expression is not in %s any more" % name)
        scope = {}
        exec(src.replace(old, new), dict(vars(F8)), scope)
        fns[name] = scope[name]
    return fns["forward_plan"], fns["backward_plan"]


def _table_mismatches(mutate=None):
    forward_plan, backward_plan = _plans(mutate)
    bad, seen = [], 0
    for inp in itertools.product((0, 1), repeat=6):
        f8f, f8w, tg, tr, cal, sc = inp
        if (f8f, f8w) == (0, 0):
            want = BACKWARD_ONLY[(f8f, f8w, tg)]
        else:
            want = (True,) + DRY_AND_UPDATE[(tr, cal, sc)] + (FP8_MODE[(f8f, f8w)], False)
        got = forward_plan(*(bool(x) for x in inp))
        seen += 1
        if tuple(got) != want or not all(type(g) is type(w) for g, w in zip(got, want)):
            bad.append(("forward", inp, tuple(got), want))
    assert seen == 64
    for inp, want in BACKWARD.items():
        got = backward_plan(*(bool(x) for x in inp))
        if tuple(got) != want:
            bad.append(("backward", inp, tuple(got), want))
    return bad


def test_forward_and_backward_plans_follow_the_table():
    assert _table_mismatches() == []


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_table_catches_each_mutant(mutant):
    bad = _table_mismatches(mutate=mutant)
    assert bad, mutant
    assert {b[0] for b in bad} == {MUTANTS[mutant][0].split("_")[0]}, bad     # ... and only in the function that was mutated


# ------------------------------------------------------------------------------------------- window counter
def test_scale_set_counter_resets_on_every_window_th_call():
    count, resets = 0, []
    for call in range(1, 10):
        count, reset = F8.next_reset(count, 4)
        assert count == call
        resets.append(reset)
    assert resets == [0, 0, 0, 1, 0, 0, 0, 1, 0]          # the counter moves first: calls 4 and 8 of 9
    assert F8.AMAX_WINDOW == 256 and F8.next_reset(255) == (256, 1) and F8.next_reset(256) == (257, 0) and F8.next_reset(0) == (1, 0)
    from crct.model import CrctModel
    assert CrctModel.FP8_AMAX_WINDOW is F8.AMAX_WINDOW
