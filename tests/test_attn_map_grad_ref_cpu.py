"""The yardstick of the attention-map backward (tests/attn_map_grad_ref.py) proved on the CPU -- the emulator of the kernel's documented
arithmetic stays inside the derived budget on every shape of the GPU test, every named mutant leaves it on at least one of them, torch
autograd through an fp64 softmax agrees with the reference -- and the C ABI of the feature: crct_attention_probs_bwd and
crct_engine_set_attention_map_grads are exported and bound, the ABI version is still 7, CrctAttnMapGrad has 24 bytes, and both refuse
what they cannot take before anything touches a GPU.  No GPU."""
import ctypes as C
import functools
import math

import pytest
import torch

import attention_ref as AR
import attn_map_grad_ref as MR
import dropout_ref as DR
from crct import lib as L

SEED, SITE = 5151, 11
# the entry point this yardstick is for: a library without it has nothing to hold to the budget, and this file does not load
BWD_RES, BWD_ARGS = L.PROTOTYPES["crct_attention_probs_bwd"]


@functools.lru_cache(maxsize=None)
def _case(family, shape, p, acc):
    B, heads, Tq, Tk, d = shape
    # mask_offset 1: batch row 0 of the masks family is the fully masked one (mask_row kind 1), at every B
    q, k, km, G, dq0, dk0 = MR.make_case(family, B, heads, Tq, Tk, d, seed=Tq + Tk, mask_offset=1)
    keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
    old = (dq0, dk0) if acc else (None, None)
    return (q, k, km, G), keep, old, MR.reference(q, k, km, G, MR.C_SCALE, heads, d, keep=keep, p=p, dq_old=old[0], dk_old=old[1])


def _ratio(family, shape, p, acc, mutate=None):
    (q, k, km, G), keep, old, (ref, budget) = _case(family, shape, p, acc)
    em = MR.emulate(q, k, km, G, MR.C_SCALE, shape[1], shape[4], keep=keep, p=p, dq_old=old[0], dk_old=old[1], mutate=mutate)
    return max(float(MR.ratio(e, r, b).max()) for e, r, b in zip(em, ref, budget))


@pytest.mark.parametrize("family", AR.FAMILIES)
def test_unmutated_emulator_stays_within_the_budget(family):
    """Every shape, p in {0, 0.1}, accumulate 0 and 1: every element of dq and dk of the emulator within its budget."""
    worst = 0.0
    for shape in MR.SHAPES:
        for p in (0.0, 0.1):
            for acc in (False, True):
                r = _ratio(family, shape, p, acc)
                worst = max(worst, r)
                assert r <= 1.0, "%s %s p=%g accumulate=%d: %.3f of the budget" % (family, shape, p, acc, r)
    print("%-10s largest |emulator - fp64| / budget %.2f" % (family, worst))


# mutant -> (family, p, accumulate): where it acts (the dropout mutants need p > 0, pad_masked a fully masked batch row, overwrite old values)
MUTANT_CASES = {
    "delta_dropped": ("flat", 0.0, False), "keep_ignored_on_g": ("flat", 0.1, False), "dropout_scale_once": ("flat", 0.1, False),
    "scale_missing": ("flat", 0.0, False), "ragged_last_key": ("flat", 0.0, False), "dk_last_qtile": ("flat", 0.0, False),
    "pad_masked": ("masks", 0.0, False), "overwrite": ("flat", 0.0, True),
}


@pytest.mark.parametrize("mutant", MR.MUTANTS)
def test_every_mutant_exceeds_the_budget(mutant):
    """Each wrong kernel of attn_map_grad_ref.emulate leaves the budget on at least one shape, where the clean emulator stays inside on all."""
    family, p, acc = MUTANT_CASES[mutant]
    out = []
    for shape in MR.SHAPES:
        assert _ratio(family, shape, p, acc) <= 1.0
        if _ratio(family, shape, p, acc, mutate=mutant) > 1.0:
            out.append(shape)
    print("%-20s leaves the budget on %d of %d shapes" % (mutant, len(out), len(MR.SHAPES)))
    assert out, "%s stays inside the budget on every shape" % mutant


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(MR.MUTANTS) and len(MR.MUTANTS) >= 8


@pytest.mark.parametrize("shape", [(2, 2, 5, 7, 32), (1, 3, 17, 33, 48), (1, 2, 36, 20, 128)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_autograd_through_an_fp64_softmax_agrees_with_the_reference(shape, p):
    """loss = sum(c G o M), M = keep / (1 - p) o softmax(q k^T / sqrt(d) + (1 - keymask) * -10000) in fp64 under torch.autograd: its
    gradients with respect to q and k are the reference's dq and dk (accumulate 0) to 1e-9 of the largest element."""
    B, heads, Tq, Tk, d = shape
    q, k, km, G, _, _ = MR.make_case("flat", B, heads, Tq, Tk, d, seed=3)
    keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
    (dq, dk), _ = MR.reference(q, k, km, G, MR.C_SCALE, heads, d, keep=keep, p=p)
    qa, ka = q.double().requires_grad_(True), k.double().requires_grad_(True)
    qh = qa.reshape(B, Tq, heads, d).permute(0, 2, 1, 3)
    kh = ka.reshape(B, Tk, heads, d).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d) + (1.0 - km.double())[:, None, None, :] * -10000.0
    M = torch.softmax(s, -1) * MR._keep(keep, B, heads, Tq, Tk).double() / (1.0 - p)
    (MR.C_SCALE * G.double() * M).sum().backward()
    for got, ref, name in ((qa.grad, dq, "dq"), (ka.grad, dk, "dk")):
        assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), name


# ------------------------------------------------------------------------------------------- the C ABI, without a GPU
P = 64          # stands for a 16-byte aligned device address: a call that passes validation is never made here


def test_symbols_are_exported_and_mirrored():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("crct_attention_probs_bwd", "crct_engine_set_attention_map_grads"):
        assert hasattr(raw, name), name
        assert name in L.PROTOTYPES, name
    res, args = BWD_RES, BWD_ARGS
    assert res is C.c_int and len(args) == 23 and args[-1] is L.vp and args[4] is L.c_f32
    res, args = L.PROTOTYPES["crct_engine_set_attention_map_grads"]
    assert res is C.c_int and len(args) == 3
    assert C.sizeof(L.AttnMapGrad) == 24 and L.AttnMapGrad.d_probs.offset == 16
    assert L.load().crct_abi_version() == 7                 # new entry points and one new struct only


def _call(lib, g=P, dq=P, dk=P, scratch=P, c=1.0, Tq=20, Tk=36, d=32, ldq=3 * 64 + 8, ldk=3 * 64 + 8, lddq=3 * 64, lddk=3 * 64):
    return lib.crct_attention_probs_bwd(P, P, P, g, c, dq, dk, scratch, 1, 2, 2, Tq, Tk, d, ldq, ldk, lddq, lddk, 0, 1.0, 0, 0, None)


@pytest.mark.parametrize("kw, word", [
    (dict(Tk=513), b"must be in [1,512]"), (dict(Tq=0), b"must be in [1,512]"),
    (dict(d=72, ldq=3 * 144 + 8, ldk=3 * 144 + 8, lddq=3 * 144, lddk=3 * 144), b"multiple of 8 in [8,64]"), (dict(d=20), b"multiple of 8 in [8,64]"),
    (dict(dq=None), b"null dq / dk"), (dict(g=None), b"null q / k / keymask / d_probs"), (dict(scratch=None), b"null statistics scratch"),
    (dict(ldq=3 * 64 + 4), b"multiples of 8"), (dict(lddk=32), b"at least heads * d"), (dict(lddq=3 * 64 + 2), b"multiples of 4"),
    (dict(dk=P + 4), b"8-byte aligned"), (dict(c=float("inf")), b"must be finite"),
])
def test_attention_probs_bwd_refuses_what_it_cannot_take(kw, word):
    lib = L.load()
    assert _call(lib, **kw) != 0
    msg = lib.crct_last_error()
    assert b"attention_probs_bwd:" in msg and word in msg, msg


def test_engine_setter_refuses_a_null_engine():
    lib = L.load()
    assert lib.crct_engine_set_attention_map_grads(None, None, 0) != 0
    assert b"engine_set_attention_map_grads: null engine" in lib.crct_last_error()


def test_python_surface_exists():
    from crct import ops
    from crct.engine import StepEngine
    from crct.model import CrctModel
    assert callable(ops.attention_probs_bwd) and callable(StepEngine.set_attention_map_grads) and hasattr(CrctModel, "_attention_map_keys")
