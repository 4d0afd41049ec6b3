"""The exactness claim behind the bit-for-bit GEMM tests (tests/gemm_ref.py), proved on the CPU: for operands the generators accept,
fp32 sums of the products in forward, reverse and blocked (K-tile, split-K-slab) order all equal the fp64 product bit for bit, and a
generator asked to leave the exact regime raises."""
import numpy as np
import pytest
import torch

import gemm_ref as GR


def _fp32_orders(a, b):
    """fp32 sums over k of a[m][k] * b[n][k] (a [M][K], b [N][K] fp64, exact products) in several orders: {name: [M][N] fp64}."""
    p = (a[:, None, :] * b[None, :, :]).numpy()                      # [M][N][K] exact products (fp64)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p), "a product is not exact in fp32"
    K = p.shape[-1]
    out = {}
    acc = np.zeros(p.shape[:2], np.float32)
    for k in range(K):
        acc = acc + p32[:, :, k]
    out["forward"] = acc
    acc = np.zeros(p.shape[:2], np.float32)
    for k in reversed(range(K)):
        acc = acc + p32[:, :, k]
    out["reverse"] = acc
    for blk, S in ((64, 1), (32, 3), (128, 8)):
        # K tiles of `blk` summed in order inside S slices of uneven length, the slices summed in slice order (the split-K reducer)
        tiles = [p32[:, :, k:k + blk].sum(-1, dtype=np.float32) for k in range(0, K, blk)]
        bounds = np.linspace(0, len(tiles), S + 1).astype(int)
        slabs = [np.sum(tiles[bounds[s]:bounds[s + 1]], axis=0, dtype=np.float32) for s in range(S)]
        acc = np.zeros(p.shape[:2], np.float32)
        for s in slabs:
            acc = acc + s
        out["blocked %d / %d" % (blk, S)] = acc
    acc = np.zeros(p.shape[:2], np.float32)
    for k in np.random.default_rng(0).permutation(K):                 # any order at all
        acc = acc + p32[:, :, k]
    out["shuffled"] = acc
    return {k: torch.from_numpy(v.astype(np.float64)) for k, v in out.items()}


@pytest.mark.parametrize("kind,K,amax,bmax,ea,eb", [
    ("bf16", 3072, 48, 48, -3, -5),     # the largest bf16 contraction of the GPU tests, at its magnitudes
    ("bf16", 1601, 64, 64, 0, -7),      # the register-staged weight gradients' longest R
    ("bf16", 776, 128, 96, 2, -9),
    ("e4m3", 2048, 16, 16, -3, -2),     # fp8 forward at the 2^20 bound
    ("e5m2", 2880, 8, 16, -4, -3),      # fp8 data / weight gradient: e5m2 x e4m3
])
def test_fp32_sums_of_generated_operands_are_the_fp64_product(kind, K, amax, bmax, ea, eb):
    kb = "e4m3" if kind == "e5m2" else kind
    extra = 1 << 19 if kind == "bf16" else 0                           # bias / addend / prefilled output of the bf16 tests
    a, b = GR.operands(6, 5, K, amax, bmax, seed=K, ea=ea, eb=eb, kind=kind, extra=extra, kind_b=kb)   # e5m2 A: an e4m3 B
    # the worst case of the bound, not only random signs: every product at its largest magnitude, all of one sign
    a[0] = amax * 2.0 ** ea
    b[0] = bmax * 2.0 ** eb
    ref = GR.ref_nt(a, b)
    assert float(ref[0, 0]) == K * amax * bmax * 2.0 ** (ea + eb)
    for name, got in _fp32_orders(a, b).items():
        assert torch.equal(got, ref), (kind, name)
    # the values are what the kernel's operand types hold
    if kind == "bf16":
        assert torch.equal(GR.bf16(a), a) and torch.equal(GR.bf16(b), b)
    else:
        q = GR.e4m3 if kind == "e4m3" else GR.e5m2
        assert torch.equal(q(a / 2.0 ** ea), a / 2.0 ** ea) and torch.equal(GR.e4m3(b / 2.0 ** eb), b / 2.0 ** eb)
    assert bool((a != 0).all()) and bool((b != 0).all())


def test_generators_refuse_to_leave_the_exact_regime():
    GR.check_exact(3072, 48, 48, 1 << 19)
    with pytest.raises(GR.ExactnessError):
        GR.operands(4, 4, 4096, 64, 64, seed=1)                        # 2^24 exactly
    with pytest.raises(GR.ExactnessError):
        GR.check_exact(3072, 48, 48, 1 << 24)                          # the epilogue's additions count
    with pytest.raises(GR.ExactnessError):
        GR.operands(4, 4, 2048, 16, 32, seed=1, kind="e4m3")           # fp8: 2^20
    with pytest.raises(GR.ExactnessError):
        GR.ints((3, 3), 17, 0, "e4m3")                                 # 17 is not an e4m3 value
    with pytest.raises(GR.ExactnessError):
        GR.ints((3, 3), 9, 0, "e5m2")
    with pytest.raises(GR.ExactnessError):
        GR.ints((3, 3), 257, 0, "bf16")


def test_a_sum_beyond_the_bound_does_depend_on_the_order():
    # the bound is not slack: one step past it, fp32 sums in different orders disagree
    K = 4200
    a = torch.full((1, K), 63.0)
    b = torch.full((1, K), 65.0)              # odd products: a sum past 2^24 falls between two fp32 numbers
    sums = _fp32_orders(a, b)
    assert not torch.equal(sums["forward"], GR.ref_nt(a, b))


def test_epilogue_restatement():
    acc = torch.tensor([[257.0, -3.0, 4.0, 511.0]])
    bias = torch.tensor([0.0, 1.0, -8.0, 2.0])
    r = GR.epilogue(acc, bias=bias, act="relu", out="bf16")
    assert r["pre"].tolist() == [[256.0, -2.0, -4.0, 512.0]]            # 257: a tie, to even
    assert r["y"].tolist() == [[256.0, 0.0, 0.0, 512.0]]
    keep = torch.tensor([[True, False, True, True]])
    r = GR.epilogue(acc, keep=keep, drop_scale=2.0, addend=torch.tensor([[1.0, 1.0, 1.0, 1.0]]), prev=torch.ones(1, 4), out="f32")
    assert r["y"].tolist() == [[516.0, 2.0, 10.0, 1024.0]]
    assert GR.bf16_ties(torch.tensor([257.0, 258.0, 259.0, 514.0, 516.0])) == 3
    r = GR.epilogue(torch.tensor([[100.0, -1000.0]]), q_scale=4.0, q_kind="e4m3")
    assert r["q"].tolist() == [[384.0, -448.0]] and r["amax"] == 1000.0   # 400 -> 384 (to even), -4000 saturates
