"""CPU: the C ABI of the global-norm gradient clipping (crct_grad_sumsq / crct_grad_norm_finalize / crct_scale_runs): the symbols
are exported and bound, and each refuses null or negative arguments with a message before anything touches a GPU.  No GPU compute."""
import ctypes as C

import pytest

from crct import lib as L

NAMES = ("crct_grad_sumsq", "crct_grad_norm_finalize", "crct_scale_runs")
P = 64          # stands for a device address: a call that passes validation is never made here


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and args[-1] is L.vp          # int status, stream last
    assert len(L.PROTOTYPES["crct_grad_sumsq"][1]) == 11
    assert len(L.PROTOTYPES["crct_grad_norm_finalize"][1]) == 11
    assert len(L.PROTOTYPES["crct_scale_runs"][1]) == 9
    assert L.load().crct_abi_version() == 7                 # new entry points only: no struct or prototype changed


def _refused(rc, lib, word):
    assert rc != 0
    msg = lib.crct_last_error()
    assert word in msg, msg


@pytest.mark.parametrize("null_at", [2, 3, 4, 5])
def test_grad_sumsq_refuses_a_null_table(null_at):
    lib = L.load()
    a = [P, None, P, P, P, P, 3, P, 0, 0, None]          # g_f32, g_bf16, seg_off, seg_len, blk_seg, blk_off, n_blk, partials, kind, max_wg, stream
    a[null_at] = None
    _refused(lib.crct_grad_sumsq(*a), lib, b"grad_sumsq: null chunk table")


def test_grad_sumsq_refuses_other_bad_arguments():
    lib = L.load()
    ok = [P, None, P, P, P, P, 3, P, 0, 0, None]
    for pos, val, word in ((7, None, b"null partials"), (0, None, b"no gradient buffer"), (6, -1, b"n_blk"), (8, 2, b"norm_kind"),
                           (9, -1, b"max_workgroups")):
        a = list(ok)
        a[pos] = val
        _refused(lib.crct_grad_sumsq(*a), lib, word)


def test_grad_norm_finalize_refuses_bad_arguments():
    lib = L.load()
    ok = [P, P, 3, 2, 0, 1.0, None, None, P, P, None]     # partials, blk_seg, n_blk, n_seg, kind, max_norm, grad_scale, mul, out, seg_norm, stream
    for pos, val, word in ((8, None, b"null out"), (0, None, b"null partials"), (1, None, b"null blk_seg"), (2, -1, b"negative count"),
                           (3, -1, b"negative count"), (4, 5, b"norm_kind"), (5, -1.0, b"negative max_norm")):
        a = list(ok)
        a[pos] = val
        _refused(lib.crct_grad_norm_finalize(*a), lib, word)


def test_scale_runs_refuses_bad_arguments():
    lib = L.load()
    ok = [P, P, P, P, P, P, 3, 0, None]                   # g_f32, coef, seg_off, seg_len, blk_seg, blk_off, n_blk, max_wg, stream
    for pos, word in ((0, b"null gradient buffer or coefficient"), (1, b"null gradient buffer or coefficient"), (2, b"null chunk table"),
                      (3, b"null chunk table"), (4, b"null chunk table"), (5, b"null chunk table")):
        a = list(ok)
        a[pos] = None
        _refused(lib.crct_scale_runs(*a), lib, word)
    for pos, word in ((6, b"n_blk"), (7, b"max_workgroups")):
        a = list(ok)
        a[pos] = -1
        _refused(lib.crct_scale_runs(*a), lib, word)


def test_optimizer_surface_exists():
    from crct import optim
    assert callable(optim.clip_grad_norm_)
    for name in ("clip_grad_norm_", "grad_norms", "grad_norm_names"):
        assert hasattr(optim.FusedAdamW, name), name
