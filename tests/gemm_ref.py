"""Exact-operand references for the GEMM kernels (csrc/gemm.hip): integer-valued operands scaled by powers of two, and the fused
epilogue restated in the kernels' order on top of an fp64 product.

Why the checks built on this module can be bit for bit: the kernels multiply bf16 (or e4m3 / e5m2) operands exactly and add the
products in fp32.  When every operand is an integer multiple of 2^ea (A) or 2^eb (B) and every partial sum, in units of
u = 2^(ea + eb), stays below 2^24, every fp32 addition is exact -- whatever the tile, the split of K or the order of the additions --
and the fp32 accumulator IS the fp64 product.  For the fp8 kernels the bound is 2^20: whether the gfx950 fp8 MFMAs accumulate at
full fp32 precision has not been measured, and 2^20 keeps the sums exact for an accumulator 4 bits narrower.  The generators below
assert that bound for the largest partial sum a launch can meet (K * max|a| * max|b| plus every value the epilogue adds to it), so a
test cannot quietly leave the exact regime.

Every operand entry is non-zero: a dropped, doubled or misplaced product then changes the exact result.

The epilogue (`epilogue`) follows gemm_epilogue_staged / gemm_epilogue: * alpha, + bias, store the pre-activation (bf16), act,
* act'(dact_src), dropout (keep ? v * scale : 0), + addend (bf16 or fp32), then + the old output (accumulate) and the store as fp32
or bf16.  Values are rounded to fp32 after every step (exact in the exact regime) and to bf16 / e4m3 / e5m2 only where the kernel
stores.  The CPU test (tests/test_gemm_ref_cpu.py) checks the exactness claim itself.
"""
import math

import numpy as np
import torch

EXACT_BITS = {"bf16": 24, "e4m3": 20, "e5m2": 20}
# largest integer magnitude every value of which the format holds exactly (8 / 4 / 3 significant bits)
INT_MAX = {"bf16": 256, "e4m3": 16, "e5m2": 8}


class ExactnessError(ValueError):
    pass


def check_exact(K, amax, bmax, extra=0, kind="bf16"):
    """Raise unless K * amax * bmax + extra < 2^EXACT_BITS[kind] (all in units of the product's scale).  Returns the bound."""
    total = int(K) * int(amax) * int(bmax) + int(extra)
    if total >= 1 << EXACT_BITS[kind]:
        raise ExactnessError("partial sums up to %d reach 2^%d: fp32 accumulation of %s operands is no longer exact"
                             % (total, EXACT_BITS[kind], kind))
    return total


def ints(shape, vmax, seed, kind="bf16"):
    """fp64 CPU tensor of non-zero integers in [-vmax, vmax] (uniform magnitude, random sign), exactly representable in `kind`."""
    if not 1 <= vmax <= INT_MAX[kind]:
        raise ExactnessError("|values| <= %d are not all exact in %s" % (vmax, kind))
    g = np.random.default_rng(seed)
    mag = g.integers(1, int(vmax) + 1, size=shape)
    sign = np.where(g.random(size=shape) < 0.5, -1, 1)
    return torch.from_numpy((mag * sign).astype(np.float64))


def operands(rows_a, rows_b, K, amax, bmax, seed, ea=0, eb=0, kind="bf16", extra=0, kind_b=None):
    """(A, B): [rows_a][K] integers * 2^ea and [rows_b][K] integers * 2^eb in fp64 (CPU), after check_exact with `extra` units of
    2^(ea + eb) for what the epilogue adds.  kind_b: B's type when it differs from A's (e5m2 x e4m3).  Lay them out (transpose,
    pad) and cast them to the kernel's type as the test needs."""
    check_exact(K, amax, bmax, extra, kind)
    return ints((rows_a, K), amax, seed, kind) * 2.0 ** ea, ints((rows_b, K), bmax, seed + 1, kind_b or kind) * 2.0 ** eb


def unit_ints(shape, vmax, seed, unit, kind="bf16"):
    """Epilogue inputs (bias, addend, prefilled output): non-zero integers in [-vmax, vmax] times `unit` (fp64, CPU)."""
    return ints(shape, vmax, seed, kind) * unit


# ------------------------------------------------------------------------------------------- fp64 products of the three layouts
def ref_nt(a, b):
    """forward: C[m][n] = sum_k a[m][k] b[n][k]  (ta = tb = 0)."""
    return a.double() @ b.double().t()


def ref_tb(a, bt):
    """data gradient: bt = B stored [K][N] (tb = 1)."""
    return a.double() @ bt.double()


def ref_tt(at, bt):
    """weight gradient: at = A stored [K][M], bt = B stored [K][N] (ta = tb = 1): C = at^T bt."""
    return at.double().t() @ bt.double()


def strided(x, ld, rows=None, fill=0.0):
    """x [r][c] placed in the first c columns of a [rows or r][ld] buffer filled with `fill` (a strided operand / output)."""
    r, c = x.shape
    out = torch.full((rows or r, ld), float(fill), dtype=x.dtype, device=x.device)
    out[:r, :c] = x
    return out


# ------------------------------------------------------------------------------------------- roundings
def f32(x):
    return x.to(torch.float32).to(torch.float64)


def bf16(x):
    """Round to nearest even bf16, through fp32 (exact for the fp32-representable values the kernels round)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def e4m3(x):
    """OCP e4m3 of x, saturating at +-448 (f8_clamp), round to nearest even."""
    return x.to(torch.float32).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float64)


def e5m2(x):
    return x.to(torch.float32).clamp(-57344.0, 57344.0).to(torch.float8_e5m2).to(torch.float64)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


ACTS = {"none": lambda v: v, "relu": lambda v: torch.clamp_min(v, 0.0), "gelu": gelu64, "tanh": torch.tanh,
        "leaky": lambda v: torch.where(v > 0, v, 0.01 * v)}
DACTS = {"gelu": gelu_grad64, "relu": lambda s: (s > 0).double(), "leaky": lambda s: torch.where(s > 0, 1.0, 0.01).double(),
         "tanh": lambda s: 1.0 - s * s}


def epilogue(acc, alpha=1.0, bias=None, act="none", dact=None, dact_src=None, keep=None, drop_scale=1.0, addend=None,
             prev=None, out="bf16", q_scale=None, q_kind=None):
    """The kernel's epilogue on the exact fp64 accumulator `acc` [M][N] (tensors on any one device, fp64 or castable).
    Returns dict(pre=bf16 pre-activation, y=stored output (fp64 holding an `out` value), v=the value before the store rounding,
    q=the fp8 copy (q_kind 'e4m3' / 'e5m2', quantised with q_scale), amax=max |v| over the output)."""
    v = f32(acc.double())
    if alpha != 1.0:
        v = f32(v * alpha)
    if bias is not None:
        v = f32(v + bias.double()[None, :])
    pre = bf16(v)
    v = ACTS[act](v)
    if dact is not None:
        v = v * DACTS[dact](dact_src.double())
    if keep is not None:        # one fp32 multiply by the kernel's fp32 scale (exact for p = 0.5 / 0.75 on exact values)
        v = torch.where(keep.bool(), f32(v * float(np.float32(drop_scale))), torch.zeros_like(v))
    if addend is not None:
        v = v + addend.double()
    res = dict(pre=pre, v=v)
    if q_kind is not None:
        res["q"] = (e4m3 if q_kind == "e4m3" else e5m2)(v * q_scale)
        res["amax"] = float(v.abs().max())
    if prev is not None:
        v = v + prev.double()
    res["y"] = f32(v) if out == "f32" else bf16(v)
    return res


def bf16_ties(y):
    """How many of the fp64 values y (each representable in fp32) lie exactly halfway between two bf16 numbers."""
    y = y.double()
    lo = y.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    step = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126))) - 7)
    return int(((y - lo).abs() == step / 2).sum())
