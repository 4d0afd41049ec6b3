"""CPU: the C boundary of the sequence outputs (crct_engine_sequence_outputs / crct_engine_set_output_grads and their two kernels'
standalone entries) -- exported, mirrored in crct.lib.PROTOTYPES, under the unchanged ABI number, with the request struct's size."""
import ctypes as C
import os

from crct import lib as L

NEW = ("crct_layernorm_rows_f32", "crct_hidden_grad_add", "crct_engine_sequence_outputs", "crct_engine_set_output_grads")


def test_new_symbols_are_exported_and_mirrored():
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in L.PROTOTYPES, "%s has no prototype in crct.lib" % name
        assert L.PROTOTYPES[name][0] is C.c_int
    # argument counts as include/crct_hip.h declares them (the trailing one is the stream)
    assert [len(L.PROTOTYPES[n][1]) for n in NEW] == [10, 5, 9, 2]
    assert L.PROTOTYPES["crct_hidden_grad_add"][1][2] is C.c_float and L.PROTOTYPES["crct_hidden_grad_add"][1][3] is C.c_int64
    assert L.load().crct_abi_version() == 7


def test_output_grads_struct_is_two_pointers():
    assert C.sizeof(L.OutputGrads) == 16
    assert [f[0] for f in L.OutputGrads._fields_] == ["d_seq_t", "d_seq_v"]
    assert L.OutputGrads.d_seq_t.offset == 0 and L.OutputGrads.d_seq_v.offset == 8
