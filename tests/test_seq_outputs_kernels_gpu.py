"""The two kernels behind the sequence outputs, through the C ABI (-m gpu).

crct_hidden_grad_add: x = bf16(float(x) + c * g) in place, bit for bit against the same two fp32 torch operations and the cast.

crct_layernorm_rows_f32: the fp32 value of a LayerNorm output rebuilt from the rows it normalised and the statistics it stored --
bit-identical to the fp32 copy crct_layernorm_fwd_args writes from the same input, its bf16 rounding bit-identical to that call's bf16
output, and per element against fp64 evaluated FROM THE KERNEL'S OWN mean / rstd.  Budget of that last check, derived, not measured: with
u = 2^-24 and exact fp32 inputs, ln_value rounds three times -- d = fl(x - mean) (relative u), t = fl(d * rstd) (relative u more) and
y = fl(gamma * t + beta), ONE fused multiply-add (relative u of y) -- so |y - y64| <= 2 u |gamma xhat| + u |y64| to first order, which
3 u (|gamma xhat| + |beta|) covers with room for the second-order terms; the comparison itself rounds y64 to fp32 once more: + u |y64|.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import lib as L                          # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stream():
    return L.current_stream()


# ------------------------------------------------------------------------------------------------ hidden_grad_add
@pytest.mark.parametrize("c", [1.0, 0.5, 3.1, 65536.0])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4097, 3 * 31 * 768])
def test_hidden_grad_add_matches_two_fp32_torch_ops_bit_for_bit(n, c):
    lib = L.load()
    gen = torch.Generator().manual_seed(1000 + n)
    guard = 64
    x = (torch.randn(n + guard, generator=gen) * 0.05).to(torch.bfloat16)
    g = torch.randn(n + guard, generator=gen) * (0.05 / c)
    # special operands, as far as n has room for them (slot k of `special` lands on element k):
    #   +-0 with a zero and a non-zero addend; bf16 subnormals (2^-133, the smallest, and 2^-127 - 2^-133) against a tiny addend;
    #   1 + c g = 1 + 2^-8 and 1 + 2^-7 + 2^-8: exact ties between two bf16 values (c a power of two), one rounding down to even, one up;
    #   one +inf and one NaN in g
    sub_lo, sub_hi = 2.0 ** -133, 2.0 ** -127 - 2.0 ** -133
    special = [(0.25, float("inf")), (0.5, float("nan")), (sub_lo, 0.0), (-sub_hi, 2.0 ** -130 / c), (0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0),
               (1.0, 2.0 ** -8 / c), (1.0 + 2.0 ** -7, 2.0 ** -8 / c), (-1.0, -(2.0 ** -8) / c), (0.0, 1.0 / c), (sub_hi, -sub_hi / c)]
    if n >= 7:                                       # as many as fit in front of n, the non-finite pair first
        for k, (xv, gv) in enumerate(special[:n]):
            x[k], g[k] = xv, gv
        assert float(x[2].float()) == sub_lo and float(x[3].float()) == -sub_hi      # the subnormals survive the host-side cast
    else:
        x[0], g[0] = special[7]
    want = (x[:n].float() + torch.tensor(c, dtype=torch.float32) * g[:n]).bfloat16()
    xd, gd = x.to(DEV), g.to(DEV)
    assert xd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
    L.check(lib.crct_hidden_grad_add(xd.data_ptr(), gd.data_ptr(), c, n, _stream()), "hidden_grad_add")
    torch.cuda.synchronize()
    got = xd.cpu()
    assert torch.equal(bits(got[n:]), bits(x[n:])), "the guard band behind n was written"
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got[:n].float()), nan), "a NaN of g did not arrive (or one appeared)"
    assert torch.equal(bits(got[:n])[~nan], bits(want)[~nan]), ((bits(got[:n]) != bits(want)) & ~nan).nonzero()[:8].flatten().tolist()
    if n >= 7:
        assert int(nan.sum()) == 1 and bool(torch.isinf(got[:n].float()).any())            # each of the two arrived


def test_hidden_grad_add_refuses_misaligned_buffers():
    lib = L.load()
    x = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    g = torch.zeros(64, device=DEV)
    assert lib.crct_hidden_grad_add(x.data_ptr() + 2, g.data_ptr(), 1.0, 8, _stream()) != 0
    assert lib.crct_hidden_grad_add(x.data_ptr(), g.data_ptr() + 4, 1.0, 8, _stream()) != 0
    assert lib.crct_hidden_grad_add(x.data_ptr(), g.data_ptr(), 1.0, 0, _stream()) == 0        # nothing to do
    torch.cuda.synchronize()
    assert float(x.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ ln_rows_f32
@pytest.mark.parametrize("s_bf16", [False, True], ids=["s_fp32", "s_bf16"])
@pytest.mark.parametrize("N", [64, 96, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 93])
def test_layernorm_rows_f32_rebuilds_the_forward_output(M, N, s_bf16):
    lib = L.load()
    gen = torch.Generator().manual_seed(7 * M + N + int(s_bf16))
    s = torch.randn(M, N, generator=gen) * 1.7 + 0.3 * torch.randn(M, 1, generator=gen)
    s = (s.to(torch.bfloat16) if s_bf16 else s).to(DEV)
    gamma = (1.0 + 0.2 * torch.randn(N, generator=gen)).to(DEV)
    beta = (0.1 * torch.randn(N, generator=gen)).to(DEV)
    y16 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    y32 = torch.zeros(M, N, device=DEV)
    mean, rstd = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    a = L.LnFwdArgs()
    a.x, a.gamma, a.beta, a.y, a.mean, a.rstd = (t.data_ptr() for t in (s, gamma, beta, y16, mean, rstd))
    a.M, a.H, a.eps, a.drop_thr, a.drop_scale, a.drop_site, a.seed = M, N, 1e-12, 0, 1.0, 0, 0
    a.x_f32, a.y_f32 = int(not s_bf16), y32.data_ptr()
    L.check(lib.crct_layernorm_fwd_args(C.byref(a), _stream()), "layernorm_fwd_args")
    guard = 32
    out = torch.full((M * N + guard,), -7.0, device=DEV)
    L.check(lib.crct_layernorm_rows_f32(s.data_ptr(), int(s_bf16), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        out.data_ptr(), M, N, _stream()), "layernorm_rows_f32")
    torch.cuda.synchronize()
    got = out[:M * N].view(M, N)
    assert float((out[M * N:] + 7.0).abs().max()) == 0.0, "written past the last row"
    assert torch.equal(bits(got), bits(y32)), "not the bits of the forward's fp32 output"
    assert torch.equal(bits(got.bfloat16()), bits(y16)), "its bf16 rounding is not the stored LayerNorm output"
    # per element against fp64 from the kernel's own statistics (budget: module docstring)
    xhat = (s.double().cpu() - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
    gx = gamma.double().cpu()[None, :] * xhat
    y64 = gx + beta.double().cpu()[None, :]
    budget = 3 * U * (gx.abs() + beta.double().cpu().abs()[None, :]) + U * y64.abs() + 1e-45
    ratio = (got.double().cpu() - y64).abs() / budget
    print("ln_rows_f32 M %d N %d %s: worst |err| / budget %.3f" % (M, N, "bf16" if s_bf16 else "fp32", float(ratio.max())))
    assert float(ratio.max()) <= 1.0, (float(ratio.max()), (ratio > 1).nonzero()[:4].tolist())
    # and the statistics are the row's: a loose sanity bound, so that the fp64 check above does not stand on nonsense
    assert float((mean.cpu() - s.float().cpu().mean(1)).abs().max()) <= 1e-5
