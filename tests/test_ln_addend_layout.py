"""The binding of the GEMMs' LayerNorm addend (CrctGemmLnAddend, crct_gemm_bf16_ln_addend, crct_engine_set_ln_addend) mirrors
include/crct_hip.h; the additions leave the ABI version where it was.  No GPU needed."""
import ctypes as C
import os
import re

from crct import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_of_the_ln_addend_binding():
    text = open(os.path.join(ROOT, "include", "crct_hip.h")).read()
    m = re.search(r"typedef struct CrctGemmLnAddend \{(.*?)\} CrctGemmLnAddend;", text, flags=re.S)
    assert m, "CrctGemmLnAddend is declared in include/crct_hip.h"
    fields = re.findall(r"const float\* (\w+);", m.group(1))
    assert fields == ["mean", "rstd", "gamma", "beta"]
    assert [f[0] for f in L.GemmLnAddend._fields_] == fields and C.sizeof(L.GemmLnAddend) == 8 * len(fields)
    lib = L.load()
    for name in ("crct_gemm_bf16_ln_addend", "crct_gemm_bf16_grouped_ln_addend", "crct_engine_set_ln_addend"):
        assert name in L.PROTOTYPES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert lib.crct_abi_version() == 7
