"""CPU: the C ABI of the weight average in the AdamW launch (crct_adamw_step_ema): the symbol is declared, exported and bound, the ABI
version and the prototype of crct_adamw_step are what they were, and a bad ema_weight or a misaligned buffer is refused with a message
before anything touches a GPU.  No GPU compute."""
import ctypes as C
import os
import re

import pytest

from crct import lib as L

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "crct_hip.h")
# the prototype of crct_adamw_step as it stood before the average existed: it must not change
ADAMW_STEP = """int crct_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16,
                    const int64_t* seg_off, const int64_t* seg_len, const float* seg_lr, const float* seg_wd,
                    const int32_t* blk_seg, const int64_t* blk_off, int64_t n_blk,
                    float beta1, float beta2, float eps, int step, const float* inv_scale_dev, const CrctAmpState* amp,
                    const CrctFp8Shadow* fp8_shadow, int max_workgroups, int zero_grads, const void* g_bf16, crct_stream_t stream);"""
P = 64          # stands for a device address: a call that passes validation is never made here


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_new_entry_point_and_keeps_the_old_prototype():
    text = _header()
    assert ADAMW_STEP in text
    m = re.search(r"int crct_adamw_step_ema\(([^;]*)\);", text)
    assert m is not None
    new_args = " ".join(m.group(1).split())
    old_args = " ".join(ADAMW_STEP[ADAMW_STEP.index("(") + 1:ADAMW_STEP.rindex(")")].split())
    # every argument of crct_adamw_step up to g_bf16, unchanged and in order, then the buffer, its weight and the stream
    assert new_args == old_args[:-len("crct_stream_t stream")] + "float* ema, float ema_weight, crct_stream_t stream"
    assert "fmaf(ema_weight, d, e)" in text and "d  = p' - e" in text              # the formula and its two rounding points


def test_symbol_is_exported_and_bound():
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "crct_adamw_step_ema") and hasattr(raw, "crct_adamw_step")
    res, args = L.PROTOTYPES["crct_adamw_step_ema"]
    old = L.PROTOTYPES["crct_adamw_step"][1]
    assert res is C.c_int and list(args) == list(old[:-1]) + [L.vp, L.c_f32, L.vp]
    lib = L.load()
    assert lib.crct_adamw_step_ema is not None
    assert lib.crct_abi_version() == 7                 # a new entry point only: no struct or prototype changed


def _args(ema, w):
    # p, g, m, v, p_bf16, seg_off, seg_len, seg_lr, seg_wd, blk_seg, blk_off, n_blk, beta1, beta2, eps, step, inv_scale, amp, fp8,
    # max_workgroups, zero_grads, g_bf16, ema, ema_weight, stream
    return [P, P, P, P, P, P, P, P, P, P, P, 3, 0.9, 0.999, 1e-8, 1, None, None, None, 0, 0, None, ema, w, None]


@pytest.mark.parametrize("w", [-0.1, 1.5, float("nan"), float("inf")])
def test_bad_ema_weight_is_refused_by_name(w):
    lib = L.load()
    assert lib.crct_adamw_step_ema(*_args(P, w)) != 0
    assert b"ema_weight" in lib.crct_last_error()


def test_misaligned_average_is_refused():
    lib = L.load()
    assert lib.crct_adamw_step_ema(*_args(P + 4, 0.1)) != 0
    assert b"16-byte aligned" in lib.crct_last_error()


def test_step_still_validated_first():
    lib = L.load()
    a = _args(P, 0.1)
    a[15] = 0
    assert lib.crct_adamw_step_ema(*a) != 0
    assert b"step must be >= 1" in lib.crct_last_error()


def test_optimizer_and_checkpoint_surface_exists():
    import inspect
    from crct import checkpoint, ops, optim
    for name in ("enable_ema", "disable_ema", "ema_reset", "ema_state_dict", "load_ema_state_dict", "swap_ema", "ema_enabled"):
        assert hasattr(optim.FusedAdamW, name), name
    assert "use_ema" in inspect.signature(checkpoint.load_model_weights).parameters
    sig = inspect.signature(ops.adamw_step).parameters
    assert sig["ema"].default is None and sig["ema_weight"].default == 0.0
