"""Kernel-level parity (-m gpu): every launcher of libcrct_hip.so, called through the C ABI, against
plain fp32 PyTorch / the CPU oracle on identical seeded inputs.

Tolerances (stated per SURVEY.md 8c): kernels take bf16 operands and accumulate in fp32, so against an
fp32 reference evaluated on the SAME bf16-rounded operands the only differences are accumulation
order and the final bf16 rounding of the output: |err| <= 1e-2 * max|ref| for bf16 outputs,
<= 2e-3 * max|ref| for fp32 outputs.  That bound is normalised by the whole output and cannot see a local error: the sections
"against fp64" below check per element -- the GEMMs bit for bit on exact operands (tests/gemm_ref.py), the row kernels within one
rounding of fp64.  The attention kernels have their per-element check in a file of their own, tests/test_attention_gpu.py: every
instantiation of the three implementations against fp64 under the budget that tests/attention_ref.py derives from the kernels'
roundings, with strided outputs in sentinel-filled buffers; the attention tests in this file keep the whole-output bound.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
from oracle import crct_oracle as O   # noqa: E402
import dropout_ref as DR              # noqa: E402

DEV = "cuda"


def bf(t):
    return t.to(torch.bfloat16)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def host_keep(seed, site, M, N, p):
    """The kernels' row-major dropout mask of (seed, site) from the host Philox copy (tests/dropout_ref.py), bool [M, N] on the GPU."""
    return torch.from_numpy(DR.keep_rowmajor(seed, site, M, N, p)).to(DEV)


# ------------------------------------------------------------------------------------------- GEMM
@pytest.fixture(params=["pipelined", "generic"], autouse=True)
def gemm_path(request):
    """Every test runs with the LDS-DMA pipelined kernel (default for K % 64 == 0) and with every GEMM forced
    through the register-staged generic kernel."""
    lib = L.load()
    lib.crct_gemm_force_generic(int(request.param == "generic"))
    yield request.param
    lib.crct_gemm_force_generic(0)


@pytest.mark.parametrize("M,N,K", [(1600, 3072, 768), (2880, 1024, 2048), (1600, 768, 3072), (80, 1024, 768),
                                   (21, 64, 96), (15, 128, 32), (300, 2304, 768)])
@pytest.mark.parametrize("tile", [-1, 0, 3, 9, 11, 12, 50])
def test_gemm_forward(M, N, K, tile):
    x, w, b = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.05, seed=2)), rand(N, seed=3)
    y = ops.gemm(x, w, M, N, K, bias=b, tile=tile)
    ref = x.float() @ w.float().t() + b
    assert rel_err(y, ref) < 1e-2
    y32 = ops.gemm(x, w, M, N, K, bias=b, out_f32=True, tile=tile)
    assert rel_err(y32, ref) < 2e-3


def test_gemm_refuses_a_configuration_that_is_not_built():
    # an explicit CrctGemmArgs.tile without a launcher is an error that names it, on either kernel path (gemm_path) -- never
    # a quiet run of another configuration
    x, w = bf(rand(1600, 768, seed=1)), bf(rand(768, 768, scale=0.05, seed=2))
    with pytest.raises(RuntimeError, match="configuration 22 is not built"):
        ops.gemm(x, w, 1600, 768, 768, tile=22)


def test_gemm_identity_asymmetric():
    # A = I with an asymmetric B catches a transposed C write (cdna_hip_programming.md section 3)
    n = 128
    eye = bf(torch.eye(n, device=DEV))
    w = bf(torch.arange(n * n, device=DEV, dtype=torch.float32).reshape(n, n) % 251 - 125)
    y = ops.gemm(eye, w, n, n, n, out_f32=True)
    assert torch.equal(y, w.float().t())


@pytest.mark.parametrize("M,N,K", [(1600, 768, 2304), (2880, 1024, 3072), (21, 64, 192), (80, 768, 1024)])
@pytest.mark.parametrize("tile", [-1, 3, 9, 12, 50])
def test_gemm_dgrad(M, N, K, tile):
    # dx[M][N=in] = dy[M][K=out] @ W[K=out][N=in]
    dy, w = bf(rand(M, K, seed=4)), bf(rand(K, N, scale=0.05, seed=5))
    add = bf(rand(M, N, seed=6))
    dx = ops.gemm(dy, w, M, N, K, tb=True, addend=add, tile=tile)
    ref = dy.float() @ w.float() + add.float()
    assert rel_err(dx, ref) < 1e-2


@pytest.mark.parametrize("R,N,K", [(1600, 768, 3072), (2880, 1024, 1024), (21, 64, 128), (80, 1024, 768), (1600, 2304, 768)])
@pytest.mark.parametrize("tile", [-1, 3, 9, 12])
def test_gemm_wgrad(R, N, K, tile):
    # dW[N=out][K=in] = dy[R][N]^T @ x[R][K]; fp32 output, accumulate
    dy, x = bf(rand(R, N, seed=7)), bf(rand(R, K, seed=8))
    out = torch.ones(N, K, device=DEV)
    ops.gemm(dy, x, N, K, R, ta=True, tb=True, lda=N, ldb=K, out=out, accumulate=True, tile=tile)
    ref = dy.float().t() @ x.float() + 1.0
    assert rel_err(out, ref) < 2e-3


@pytest.mark.parametrize("R", [1600, 2880, 80])
def test_gemm_wgrad_grouped(R):
    # the weight gradients of one layer as ONE grid (different shapes per problem); small R falls back to single launches
    shapes = [(768, 768), (2304, 768), (3072, 768), (768, 3072), (1024, 1024)]
    probs, refs = [], []
    for i, (N, K) in enumerate(shapes):
        dy, x = bf(rand(R, N, seed=20 + i)), bf(rand(R, K, seed=40 + i))
        out = torch.full((N, K), float(i), device=DEV)
        probs.append((dy, x, out))
        refs.append(dy.float().t() @ x.float() + float(i))
    ops.gemm_wgrad_grouped(probs)
    for (_, _, out), ref in zip(probs, refs):
        assert rel_err(out, ref) < 2e-3
    # and against the one-by-one launches (only the fp32 accumulation order may differ)
    if R > 96:
        for i, (dy, x, out) in enumerate(probs):
            solo = torch.full_like(out, float(i))
            ops.gemm(dy, x, out.shape[0], out.shape[1], R, ta=True, tb=True, lda=out.shape[0], ldb=out.shape[1], out=solo,
                     accumulate=True, tile=9)
            assert rel_err(out, solo) < 2e-5


@pytest.mark.parametrize("R", [1600, 2880])
def test_gemm_wgrad_with_bias_gradient(R, gemm_path):
    # rowsum_out: the bias gradient (column sums of dy) out of the weight-gradient kernel itself, single and grouped
    shapes = [(768, 3072), (2304, 768), (1024, 1024)]
    probs, refs = [], []
    for i, (N, K) in enumerate(shapes):
        dy, x = bf(rand(R, N, seed=60 + i)), bf(rand(R, K, seed=70 + i))
        out, db = torch.zeros(N, K, device=DEV), torch.full((N,), 2.0, device=DEV)
        probs.append((dy, x, out, db))
        refs.append((dy.float().t() @ x.float(), dy.float().sum(0) + 2.0))
    if gemm_path == "generic":
        # row sums exist in the LDS-DMA kernel only: with every GEMM forced through the register-staged kernel a request for them
        # is an error, single or grouped -- never a weight gradient with its bias gradient left unwritten
        with pytest.raises(RuntimeError, match="gemm"):
            ops.gemm_wgrad_grouped(probs)
        dy, x, out, db = probs[0]
        with pytest.raises(RuntimeError, match="gemm"):
            ops.gemm(dy, x, 768, 3072, R, ta=True, tb=True, lda=768, ldb=3072, out=out, accumulate=True, rowsum_out=db)
        return
    ops.gemm_wgrad_grouped(probs)
    for (_, _, out, db), (rw, rb) in zip(probs, refs):
        assert rel_err(out, rw) < 2e-3 and rel_err(db, rb) < 2e-3
    for tile in (-1, 9, 12, 3):
        dy, x, _, _ = probs[0]
        out, db = torch.zeros(768, 3072, device=DEV), torch.zeros(768, device=DEV)
        ops.gemm(dy, x, 768, 3072, R, ta=True, tb=True, lda=768, ldb=3072, out=out, accumulate=True, tile=tile, rowsum_out=db)
        assert rel_err(out, refs[0][0]) < 2e-3 and rel_err(db, refs[0][1] - 2.0) < 2e-3, tile


@pytest.mark.parametrize("M,N,K,tb", [(1600, 768, 3072, False), (1600, 768, 3072, True), (1600, 768, 2304, True), (1600, 768, 768, False),
                                      (2880, 1024, 3072, True), (1600, 768, 1024, False), (300, 1000, 1280, False), (130, 72, 512, True)])
@pytest.mark.parametrize("tile", [-1, 4, 9, 12, 15])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_gemm_split_k_matches_unsplit_and_is_reproducible(M, N, K, tb, tile, S, gemm_path):
    """CrctGemmArgs.split_k: S workgroups per output tile, slabs + ticket, the last arriver sums the slabs in slice order and
    runs the FULL epilogue (bias, pre-activation copy, GELU, dropout, residual).  Against fp32 torch within the bf16 bound,
    against the unsplit launch within the fp32 re-association bound, and twice in a row bit for bit (the summation order does not
    depend on which slice finishes last); ragged M / N edges and a K that does not divide evenly into slices included.  Split-K exists
    in the LDS-DMA kernel only: with every GEMM forced through the register-staged kernel the request runs unsplit, and must give the
    same results under the same bounds."""
    x = bf(rand(M, K, seed=1))
    w = bf(rand(K, N, scale=0.05, seed=2)) if tb else bf(rand(N, K, scale=0.05, seed=2))
    b, add = rand(N, seed=3), bf(rand(M, N, seed=6))
    ref = (x.float() @ (w.float() if tb else w.float().t())) + b + add.float()
    kw = dict(tb=tb, bias=b, addend=add, tile=tile)
    y1 = ops.gemm(x, w, M, N, K, **kw)
    ys = ops.gemm(x, w, M, N, K, split_k=S, **kw)
    ys2 = ops.gemm(x, w, M, N, K, split_k=S, **kw)
    assert rel_err(ys, ref) < 1e-2
    assert rel_err(ys, y1) < 8e-3                 # both round the same fp32 sums (up to re-association) to bf16
    assert torch.equal(ys, ys2)
    y32 = ops.gemm(x, w, M, N, K, split_k=S, out_f32=True, **kw)
    assert rel_err(y32, ref) < 2e-3
    # the epilogue extras: saved pre-activation, GELU, dropout keyed by the element index (same mask as the unsplit launch)
    pre1, pre2 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16), torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    g1 = ops.gemm(x, w, M, N, K, tb=tb, bias=b, act="gelu", preact_out=pre1, p_drop=0.1, site=5, seed=11, tile=tile)
    g2 = ops.gemm(x, w, M, N, K, tb=tb, bias=b, act="gelu", preact_out=pre2, p_drop=0.1, site=5, seed=11, tile=tile, split_k=S)
    assert rel_err(pre2, pre1) < 8e-3
    assert torch.equal(g1 == 0, g2 == 0) or float(((g1 == 0) != (g2 == 0)).float().mean()) < 1e-4      # same dropout mask (gelu(x) == 0 only by underflow)
    assert rel_err(g2, g1) < 1.5e-2


def test_gemm_split_k_under_uneven_load():
    """The hand-off must hold when the slices of a tile finish far apart and the reducer's CU has the other slabs' lines in its
    L1 from the previous launch: many back-to-back launches over the SAME slab space, beside a bandwidth hog on another stream,
    every output compared in full with the first (MI355X_MICROARCH.md: test hand-offs under uneven load, L1-warm)."""
    L.load().crct_gemm_force_generic(0)
    M, N, K = 1600, 768, 3072
    x, w = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.05, seed=2))
    hog_a = torch.empty(64 << 20, device=DEV)
    side = torch.cuda.Stream()
    ref = {S: ops.gemm(x, w, M, N, K, split_k=S, tile=t).clone() for S, t in ((2, 12), (3, 4), (4, 15))}
    torch.cuda.synchronize()
    bad = 0
    for it in range(60):
        with torch.cuda.stream(side):
            hog_a.mul_(1.0001)
        for S, t in ((2, 12), (3, 4), (4, 15)):
            y = ops.gemm(x, w, M, N, K, split_k=S, tile=t)
            bad += int(not torch.equal(y, ref[S]))
    torch.cuda.synchronize()
    assert bad == 0


def test_gemm_strided_rows():
    # CLS-row gather: A rows are hidden_states[:, 0] with row stride T*H
    B, T, H, N = 80, 20, 768, 1024
    seq = bf(rand(B * T, H, seed=9))
    w = bf(rand(N, H, scale=0.05, seed=10))
    y = ops.gemm(seq, w, B, N, H, lda=T * H, act="relu")
    ref = torch.relu(seq.view(B, T, H)[:, 0].float() @ w.float().t())
    assert rel_err(y, ref) < 1e-2
    # and the scatter back: dgrad written with ldc = T*H, accumulate
    dy = bf(rand(B, N, seed=11))
    g = torch.zeros(B * T, H, device=DEV, dtype=torch.bfloat16)
    ops.gemm(dy, w, B, H, N, tb=True, out=g, ldc=T * H)
    ops.gemm(dy, w, B, H, N, tb=True, out=g, ldc=T * H, accumulate=True)
    refg = 2 * (dy.float() @ w.float())
    assert rel_err(g.view(B, T, H)[:, 0], refg) < 1.5e-2
    assert float(g.view(B, T, H)[:, 1:].abs().max()) == 0.0


def test_gemm_epilogues():
    M, N, K = 333, 256, 128
    x, w, b = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.1, seed=2)), rand(N, seed=3)
    pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    h = ops.gemm(x, w, M, N, K, bias=b, act="gelu", preact_out=pre)
    u = x.float() @ w.float().t() + b
    assert rel_err(pre, u) < 1e-2
    assert rel_err(h, O.gelu_erf(u)) < 1e-2
    for act, fn in (("relu", torch.relu), ("leaky", lambda t: torch.nn.functional.leaky_relu(t, 0.01)), ("tanh", torch.tanh)):
        assert rel_err(ops.gemm(x, w, M, N, K, bias=b, act=act), fn(u)) < 1e-2
    # backward-through-activation epilogue: out = (x w^T) * gelu'(pre)
    g = ops.gemm(x, w, M, N, K, dact_src=pre, dact="gelu")
    pf = pre.float().requires_grad_(True)
    O.gelu_erf(pf).sum().backward()
    assert rel_err(g, (x.float() @ w.float().t()) * pf.grad) < 1.5e-2
    gl = ops.gemm(x, w, M, N, K, dact_src=h, dact="leaky")
    assert rel_err(gl, (x.float() @ w.float().t()) * torch.where(h.float() > 0, 1.0, 0.01)) < 1e-2


def test_dropout_mask_consistency_and_rate():
    # the GEMM epilogue's mask must be regenerated bit-identically by the LayerNorm backward
    M, N, K, p, site, seed = 512, 768, 64, 0.1, 17, (1 << 40) + 123456789
    x, w = bf(rand(M, K, seed=1)), bf(rand(N, K, seed=2))
    y0 = ops.gemm(x, w, M, N, K, out_f32=True)
    y1 = ops.gemm(x, w, M, N, K, out_f32=True, p_drop=p, site=site, seed=seed)
    assert bool((y0 != 0).all())
    keep = y1 != 0
    assert torch.equal(keep, host_keep(seed, site, M, N, p))      # the host Philox stream's mask, bit for bit
    rate = 1.0 - float(keep.float().mean())
    assert abs(rate - p) < 0.01
    assert torch.allclose(y1[keep], y0[keep] / (1 - p), rtol=1e-5)
    # different site / seed -> different mask
    y2 = ops.gemm(x, w, M, N, K, out_f32=True, p_drop=p, site=site + 1, seed=seed)
    assert float(((y2 != 0) != keep).float().mean()) > 0.05
    # LN backward re-applies exactly this mask to produce the producing Linear's gradient
    s = bf(rand(M, N, seed=3))
    gamma, beta = 1 + 0.1 * rand(N, seed=4), rand(N, seed=5)
    _, mean, rstd = ops.layernorm_fwd(s, gamma, beta)
    dy = bf(rand(M, N, seed=6))
    dx, dxl, _, _, dbias = ops.layernorm_bwd(dy, s, mean, rstd, gamma, want_lin=True, p_lin=p, lin_site=site, seed=seed)
    exp = torch.where(keep, dx.float() / (1 - p), torch.zeros_like(dx.float()))
    assert rel_err(dxl, exp) < 1e-2
    assert float(((dxl != 0) & ~keep).sum()) == 0
    assert torch.equal(dxl != 0, keep & (dx != 0))
    assert rel_err(dbias, dxl.float().sum(0)) < 2e-3


# ------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("M,H", [(1600, 768), (2880, 1024), (21, 64), (15, 96), (7, 2048)])
def test_layernorm_fwd_bwd(M, H):
    x = bf(rand(M, H, scale=2.0, seed=1) + 0.3)
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = O.layer_norm(xr, gr, br)
    assert rel_err(y, yr) < 1e-2
    assert rel_err(mean, xr.mean(-1)) < 1e-4
    dy = bf(rand(M, H, seed=4))
    yr.backward(dy.float())
    dx, _, dg, db, dbias = ops.layernorm_bwd(dy, x, mean, rstd, gamma)
    assert rel_err(dx, xr.grad) < 1e-2
    assert rel_err(dg, gr.grad) < 2e-3
    assert rel_err(db, br.grad) < 2e-3
    assert rel_err(dbias, xr.grad.sum(0)) < 2e-3      # column sum of the fp32 dx (before bf16 rounding)
    # accumulate flag
    dg2 = dg.clone()
    ops.layernorm_bwd(dy, x, mean, rstd, gamma, dgamma=dg2, dbeta=db.clone(), dbias=dbias.clone(), accumulate=True)
    assert rel_err(dg2, 2 * gr.grad) < 2e-3


@pytest.mark.parametrize("M,H", [(1600, 768), (2880, 1024), (21, 64), (7, 2048), (9920, 768)])
def test_layernorm_on_the_fp32_residual_stream(M, H):
    """CrctLnFwdArgs.x_f32 / y_f32, CrctLnBwdArgs.x_f32: the pre-LayerNorm rows arrive as fp32 (the GEMM epilogue left them so), the output
    is written as bf16 (GEMM operand) AND as fp32 (the next block's residual); the backward reads the fp32 rows.  Against the fp32 reference:
    the fp32 output is exact to fp32 rounding, the bf16 one is its rounding, and the statistics are those of the UNROUNDED rows."""
    x = rand(M, H, scale=2.0, seed=1) + 0.3            # fp32, not bf16-representable
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3)
    y, mean, rstd, y32 = ops.layernorm_fwd(x, gamma, beta, y_f32=True)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = O.layer_norm(xr, gr, br)
    assert float((y32 - yr).abs().max()) < 2e-5 * float(yr.abs().max())
    assert torch.equal(y, y32.to(torch.bfloat16))
    assert rel_err(mean, xr.mean(-1)) < 1e-6
    # a bf16 input with the extra fp32 output, and an fp32 input without it
    xb = bf(x)
    yb, _, _, yb32 = ops.layernorm_fwd(xb, gamma, beta, y_f32=True)
    assert torch.equal(yb, ops.layernorm_fwd(xb, gamma, beta)[0]) and torch.equal(yb, yb32.to(torch.bfloat16))
    assert torch.equal(ops.layernorm_fwd(x, gamma, beta)[0], y)
    dy = bf(rand(M, H, seed=4))
    yr.backward(dy.float())
    dx, dxl, dg, db, dbias = ops.layernorm_bwd(dy, x, mean, rstd, gamma, want_lin=True, p_lin=0.1, lin_site=3, seed=5)
    assert dx.dtype == torch.bfloat16 and rel_err(dx, xr.grad) < 1e-2
    assert rel_err(dg, gr.grad) < 2e-3 and rel_err(db, br.grad) < 2e-3
    # the dropout-masked copy: same mask as the bf16-input kernel draws for (site, seed)
    _, dxl_b, *_ = ops.layernorm_bwd(dy, xb, mean, rstd, gamma, want_lin=True, p_lin=0.1, lin_site=3, seed=5)
    assert torch.equal(dxl == 0, dxl_b == 0) or float(((dxl == 0) != (dxl_b == 0)).float().mean()) < 1e-3      # exact zeros of dx aside


def test_gemm_epilogue_on_the_fp32_residual_stream(gemm_path):
    """CrctGemmArgs.addend_f32 / c_cached: y = dropout(x W^T + b) + r with r fp32 and y written as fp32 -- the attention-output and FFN-down
    projections of the step (vilbert.py:424-428, :467-471) -- in the LDS-DMA kernel, the register-staged kernel and the split-K form."""
    for M, N, K in ((1600, 768, 768), (1600, 768, 3072), (2880, 1024, 1024), (9920, 768, 3072), (100, 64, 72)):
        x, w = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.05, seed=2))
        b, r = rand(N, seed=3), rand(M, N, seed=4)
        ref = x.float() @ w.float().t() + b + r
        out = ops.gemm(x, w, M, N, K, bias=b, addend=r, out_f32=True, c_cached=True)      # both kernels: the gemm_path fixture
        assert out.dtype == torch.float32 and rel_err(out, ref) < 2e-3, (M, N, K)
        if K % 64 == 0 and M >= 1600 and gemm_path == "pipelined":
            o2 = ops.gemm(x, w, M, N, K, bias=b, addend=r, out_f32=True, c_cached=True, split_k=2)
            assert rel_err(o2, ref) < 2e-3
        # dropout in front of the fp32 residual: the mask of (site, seed) is the bf16 form's
        o3 = ops.gemm(x, w, M, N, K, bias=b, addend=r, out_f32=True, c_cached=True, p_drop=0.1, site=7, seed=11)
        o4 = ops.gemm(x, w, M, N, K, bias=b, addend=bf(r), p_drop=0.1, site=7, seed=11)
        assert rel_err(o3, o4.float()) < 1e-2
        kept = ((o3 - r).abs() > 0)
        assert abs(float(kept.float().mean()) - 0.9) < 0.01


def test_colsum_softmax_cast():
    x = bf(rand(1600, 3072, seed=1))
    assert rel_err(ops.colsum(x, 1600, 3072), x.float().sum(0)) < 1e-4
    xs = bf(rand(37, 520, seed=2))
    assert rel_err(ops.colsum(xs, 37, 256, ld=520), xs.float()[:, :256].sum(0)) < 1e-4
    f = rand(2880, 2048, seed=3)
    assert rel_err(ops.softmax_rows(f), torch.softmax(f, -1)) < 1e-2
    f2 = rand(15, 32, seed=4) * 5
    assert rel_err(ops.softmax_rows(f2), torch.softmax(f2, -1)) < 1e-2
    # both input types element by element against fp64 (F.softmax(image_feat), vilbert.py:1476; bf16 features: bench.py --host-feat bf16):
    # 13 rows (not a multiple of 4) of which one sits at +80 (exp overflows fp32 without the max shift) and one is constant
    for F in (4, 260, 1024, 2048):
        f = rand(13, F, scale=3.0, seed=F)
        f[3] += 80.0
        f[7] = 0.25
        fb = bf(f)                                             # bf16 features, and the same values in fp32
        y32, y16 = ops.softmax_rows(fb.float()), ops.softmax_rows(fb)
        assert torch.equal(y32, y16), F                        # the same fp32 math on the same values
        ref = torch.softmax(fb.double().cpu(), -1)
        _assert_within_bf16_step(y16, ref, ref, "softmax F=%d" % F)
        ref = torch.softmax(f.double().cpu(), -1)
        _assert_within_bf16_step(ops.softmax_rows(f), ref, ref, "fp32 softmax F=%d" % F)
    w = rand(100003, seed=5)
    assert torch.equal(ops.cast_bf16(w), w.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, km, heads, d):
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh = q.float().view(B, Tq, heads, d).permute(0, 2, 1, 3)
    kh = k.float().view(B, Tk, heads, d).permute(0, 2, 1, 3)
    vh = v.float().view(B, Tk, heads, d).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d) + (1.0 - km.float())[:, None, None, :] * -10000.0
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Tq, heads * d)


@pytest.fixture(params=["mfma", "valu", "long"])
def attn_path(request):
    """Lengths <= 112 with head size 32 / 48 / 64 run on the register-resident MFMA kernels by default; 'valu' forces the fp32
    kernels, 'long' the key-tile-loop kernels of attention_long.hip (the path of everything beyond 112) wherever they apply."""
    lib = L.load()
    lib.crct_attention_force_valu(int(request.param == "valu"))
    lib.crct_attention_force_long(int(request.param == "long"))
    yield request.param
    lib.crct_attention_force_valu(0)
    lib.crct_attention_force_long(0)


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(80, 16, 20, 20, 48), (80, 16, 36, 36, 64), (80, 32, 20, 36, 32), (80, 32, 36, 20, 32),
                                             (4, 16, 100, 100, 64), (4, 32, 40, 100, 32), (4, 32, 100, 40, 32), (3, 4, 7, 5, 16),
                                             (3, 4, 5, 7, 24), (5, 16, 64, 64, 64), (5, 8, 17, 33, 48), (2, 4, 1, 1, 32),
                                             (3, 4, 16, 48, 32), (3, 4, 49, 15, 64)])
def test_attention_fwd_bwd(B, heads, Tq, Tk, d, attn_path):
    Hh = heads * d
    # q / k / v as column slices of fused [*, 3*Hh] buffers, as the step engine passes them
    bufq = bf(rand(B, Tq, 3 * Hh, seed=1))
    bufk = bf(rand(B, Tk, 3 * Hh, seed=2))
    q, k, v = bufq[:, :, :Hh], bufk[:, :, Hh:2 * Hh], bufk[:, :, 2 * Hh:]
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    for b in range(B):
        km[b, Tk - (b % 4):] = 0
    ctx = ops.attention_fwd(q, k, v, km, heads, d)
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(qr, kr, vr, km, heads, d)
    assert rel_err(ctx, ref) < 1e-2
    dctx = bf(rand(B, Tq, Hh, seed=3))
    ref.backward(dctx.float())
    dq, dk, dv = ops.attention_bwd(q, k, v, km, dctx, heads, d)
    assert rel_err(dq, qr.grad) < 1.5e-2
    assert rel_err(dk, kr.grad) < 1.5e-2
    assert rel_err(dv, vr.grad) < 1.5e-2


# Beyond 112 queries / keys: attention_long.hip.  (124, 44) is the reference's own PlotQA shape (config/plotqa.json:5-6), 256 its
# default max_seq_len (options.py:27), 512 its position table and this library's limit; ragged lengths around the 16-row tiles; padding
# keys in every batch row.
LONG_SHAPES = [(4, 16, 124, 124, 48), (4, 32, 124, 44, 32), (4, 32, 44, 124, 32), (2, 16, 256, 256, 64), (2, 16, 130, 200, 48),
               (3, 4, 113, 17, 32), (2, 4, 17, 113, 64), (2, 8, 256, 256, 32), (2, 4, 241, 129, 48), (1, 2, 1, 200, 64),
               (1, 16, 512, 512, 64), (2, 8, 300, 512, 48), (1, 4, 512, 40, 32), (1, 3, 33, 497, 64)]


# stats = "kept": the forward leaves its softmax row statistics (CrctAttnQuant.row_lse) and the backward, given them and the forward's
# output, skips its statistics sweep -- what the step engine does; "recomputed": the backward of the plain entry points (q, k, v only)
@pytest.mark.parametrize("stats", ["recomputed", "kept"])
@pytest.mark.parametrize("B,heads,Tq,Tk,d", LONG_SHAPES)
def test_attention_long_sequences_fwd_bwd(B, heads, Tq, Tk, d, stats):
    Hh = heads * d
    bufq = bf(rand(B, Tq, 3 * Hh, seed=1))
    bufk = bf(rand(B, Tk, 3 * Hh, seed=2))
    q, k, v = bufq[:, :, :Hh], bufk[:, :, Hh:2 * Hh], bufk[:, :, 2 * Hh:]
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    for b in range(B):
        km[b, Tk - 1 - 5 * b:] = 0
    lse = torch.full((B, heads, Tq), float("nan"), device=DEV) if stats == "kept" else None
    ctx = ops.attention_fwd(q, k, v, km, heads, d, row_lse=lse)
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(qr, kr, vr, km, heads, d)
    assert rel_err(ctx, ref) < 1e-2
    if lse is not None:
        # log2 of the softmax denominator in the exp2 domain = log2(e) * logsumexp of the masked, scaled scores
        sc = torch.einsum("bihd,bjhd->bhij", q.float().view(B, Tq, heads, d), k.float().view(B, Tk, heads, d)) / math.sqrt(d)
        sc = sc + (1.0 - km.float())[:, None, None, :] * -10000.0
        want = torch.logsumexp(sc, dim=-1) * math.log2(math.e)
        assert bool(torch.isfinite(lse).all()) and float((lse - want).abs().max()) < 2e-2
    dctx = bf(rand(B, Tq, Hh, seed=3))
    ref.backward(dctx.float())
    dq, dk, dv = ops.attention_bwd(q, k, v, km, dctx, heads, d, row_lse=lse, ctx=ctx if lse is not None else None)
    assert rel_err(dq, qr.grad) < 1.5e-2
    assert rel_err(dk, kr.grad) < 1.5e-2
    assert rel_err(dv, vr.grad) < 1.5e-2


def test_attention_backward_with_kept_statistics_matches_the_recomputing_one_under_dropout():
    """p = 0.1: the two backward forms regenerate the same mask (the kept-statistics form makes the dropout bits in its one sweep) and
    agree to bf16 rounding; delta_i = dctx_i . ctx_i holds WITH dropout because ctx was computed from the masked, rescaled probabilities.
    Also: row_lse and ctx come together (one without the other is an error), and both forms are bit-reproducible."""
    p = 0.1
    for B, heads, Tq, Tk, d in ((4, 16, 124, 124, 48), (3, 32, 124, 44, 32), (3, 32, 44, 124, 32), (1, 8, 300, 512, 64), (2, 4, 130, 17, 48)):
        Hh = heads * d
        q, k, v = bf(rand(B, Tq, Hh, seed=1)), bf(rand(B, Tk, Hh, seed=2)), bf(rand(B, Tk, Hh, seed=3))
        km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
        km[:, Tk - 3:] = 0
        dctx = bf(rand(B, Tq, Hh, seed=4))
        lse = torch.empty(B, heads, Tq, device=DEV)
        ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=5, seed=77, row_lse=lse)
        assert torch.equal(ctx, ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=5, seed=77))      # writing the statistics changes nothing
        plain = ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=5, seed=77)
        kept = ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=5, seed=77, row_lse=lse, ctx=ctx)
        again = ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=5, seed=77, row_lse=lse, ctx=ctx)
        for a, b, c in zip(plain, kept, again):
            assert rel_err(b, a) < 1.5e-2
            assert torch.equal(b, c)
    with pytest.raises(RuntimeError, match="come together"):
        ops.attention_bwd(q, k, v, km, dctx, heads, d, row_lse=lse)


def test_attention_long_and_short_kernels_agree_under_dropout():
    """Same Philox element numbering in attention_mfma.hip and attention_long.hip: with p = 0.1 the two must give the same
    context and gradients up to rounding (a different mask moves whole probabilities), at shapes both can take; and at a long
    shape the mask the backward regenerates is the forward's (sum_j dv = sum_i ctx for v = dctx = 1), results reproducible."""
    lib = L.load()
    p = 0.1
    for B, heads, Tq, Tk, d in ((8, 32, 20, 36, 32), (3, 16, 100, 100, 64), (4, 16, 64, 50, 48)):
        Hh = heads * d
        q, k, v = bf(rand(B, Tq, Hh, seed=1)), bf(rand(B, Tk, Hh, seed=2)), bf(rand(B, Tk, Hh, seed=3))
        km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
        km[:, Tk - 2:] = 0
        dctx = bf(rand(B, Tq, Hh, seed=4))
        outs = []
        try:
            for long in (0, 1):
                lib.crct_attention_force_long(long)
                ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=9, seed=4242)
                outs.append((ctx,) + tuple(ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=9, seed=4242)))
        finally:
            lib.crct_attention_force_long(0)
        for a, b in zip(*outs):
            assert rel_err(a, b) < 1.5e-2
    B, heads, T, d = 4, 16, 124, 48
    Hh = heads * d
    q, k = bf(rand(B, T, Hh, seed=1)), bf(rand(B, T, Hh, seed=2))
    ones = bf(torch.ones(B, T, Hh, device=DEV))
    km = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    ctx = ops.attention_fwd(q, k, ones, km, heads, d, p_drop=p, site=5, seed=99)
    assert abs(float(ctx.float().mean()) - 1.0) < 0.01 and float(ctx.float().std()) > 0.01
    assert torch.equal(ctx, ops.attention_fwd(q, k, ones, km, heads, d, p_drop=p, site=5, seed=99))
    g1 = ops.attention_bwd(q, k, ones, km, ones, heads, d, p_drop=p, site=5, seed=99)
    g2 = ops.attention_bwd(q, k, ones, km, ones, heads, d, p_drop=p, site=5, seed=99)
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))
    assert rel_err(g1[2].float().sum(1), ctx.float().sum(1)) < 1e-2


def test_attention_random_shapes_and_masks():
    """Thirty seeded random shapes (1 <= Tq, Tk <= 512, head size 32 / 48 / 64, 1 - 6 heads, 1 - 3 batch rows) with random key masks
    (at least one attended key per row; masked keys anywhere, not only at the end) through whichever MFMA path takes them, forward and
    backward against fp32 PyTorch on the same bf16 operands."""
    g = torch.Generator().manual_seed(2026)
    for case in range(30):
        B, heads = int(torch.randint(1, 4, (1,), generator=g)), int(torch.randint(1, 7, (1,), generator=g))
        Tq, Tk = int(torch.randint(1, 513, (1,), generator=g)), int(torch.randint(1, 513, (1,), generator=g))
        d = (32, 48, 64)[int(torch.randint(0, 3, (1,), generator=g))]
        Hh = heads * d
        q, k, v = (bf((torch.randn(B, T, Hh, generator=g)).to(DEV)) for T in (Tq, Tk, Tk))
        km = (torch.rand(B, Tk, generator=g) < 0.7).to(torch.uint8)
        km[torch.arange(B), torch.randint(0, Tk, (B,), generator=g)] = 1
        km = km.to(DEV)
        ctx = ops.attention_fwd(q, k, v, km, heads, d)
        qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
        ref = _attn_ref(qr, kr, vr, km, heads, d)
        assert rel_err(ctx, ref.detach()) < 1e-2, (case, B, heads, Tq, Tk, d)
        dctx = bf((torch.randn(B, Tq, Hh, generator=g)).to(DEV))
        ref.backward(dctx.float())
        for got, want, nm in zip(ops.attention_bwd(q, k, v, km, dctx, heads, d), (qr.grad, kr.grad, vr.grad), "qkv"):
            assert rel_err(got, want) < 1.5e-2, (case, nm, B, heads, Tq, Tk, d)


def test_attention_long_kernels_are_bit_reproducible_beside_other_work():
    """The long-sequence kernels have one owner and one summation order per output element (no atomics; the phases of the backward
    meet at workgroup barriers): 25 repetitions at the PlotQA lengths, with dropout, while GEMMs on another stream share the CUs,
    must reproduce the first result bit for bit -- forward, dq, dk, dv, both co-attention directions included."""
    side = torch.cuda.Stream()
    A, Bm = bf(rand(4096, 1024, seed=7)), bf(rand(1024, 1024, seed=8))
    for B, heads, Tq, Tk, d in ((8, 16, 124, 124, 48), (8, 32, 124, 44, 32), (8, 32, 44, 124, 32), (2, 16, 256, 256, 64), (1, 16, 512, 512, 64)):
        Hh = heads * d
        q, k, v = bf(rand(B, Tq, Hh, seed=1)), bf(rand(B, Tk, Hh, seed=2)), bf(rand(B, Tk, Hh, seed=3))
        dctx = bf(rand(B, Tq, Hh, seed=4))
        km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
        km[:, Tk - 7:] = 0
        first = None
        for rep in range(25):
            with torch.cuda.stream(side):
                for _ in range(4):
                    ops.gemm(A, Bm, 4096, 1024, 1024)
            out = (ops.attention_fwd(q, k, v, km, heads, d, p_drop=0.1, site=7, seed=11),) + tuple(
                ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=0.1, site=7, seed=11))
            if first is None:
                first = [t.clone() for t in out]
            else:
                for a, b in zip(out, first):
                    assert torch.equal(a, b), (rep, Tq, Tk, d)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t.float()).all()) for t in first)


def test_attention_length_and_head_size_limits_are_errors():
    lib = L.load()
    assert L.ATTN_MAX_LEN == 512
    for Tq, Tk, d in ((513, 20, 64), (20, 513, 32), (120, 120, 40), (113, 20, 16)):
        q = bf(rand(1, Tq, 2 * d, seed=1))
        k = bf(rand(1, Tk, 2 * d, seed=2))
        km = torch.ones(1, Tk, dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="attention"):
            ops.attention_fwd(q, k, k, km, 2, d)
        with pytest.raises(RuntimeError, match="attention"):
            ops.attention_bwd(q, k, k, km, q, 2, d)
    assert lib.crct_attention_quant_ok(124, 124, 48) == 1 and lib.crct_attention_quant_ok(124, 124, 40) == 0


def test_attention_identity_asymmetric(attn_path):
    # v = one-hot columns, one key unmasked per query block: ctx must reproduce v's rows exactly -> catches a transposed
    # or permuted operand in the MFMA path (cdna_hip_programming.md section 3)
    B, heads, T, d = 2, 4, 36, 64
    Hh = heads * d
    q = bf(torch.zeros(B, T, Hh, device=DEV))
    k = bf(torch.zeros(B, T, Hh, device=DEV))
    v = bf((torch.arange(B * T * Hh, device=DEV, dtype=torch.float32).reshape(B, T, Hh) % 251) - 125)
    for only in (0, 17, 35):
        km = torch.zeros(B, T, dtype=torch.uint8, device=DEV)
        km[:, only] = 1
        ctx = ops.attention_fwd(q, k, v, km, heads, d)
        assert torch.equal(ctx.float(), v[:, only:only + 1].float().expand(B, T, Hh))


def test_attention_paths_share_the_dropout_stream():
    B, heads, Tq, Tk, d, p = 8, 32, 20, 36, 32, 0.1
    Hh = heads * d
    q, k, v = bf(rand(B, Tq, Hh, seed=1)), bf(rand(B, Tk, Hh, seed=2)), bf(rand(B, Tk, Hh, seed=3))
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    dctx = bf(rand(B, Tq, Hh, seed=4))
    lib = L.load()
    outs = []
    for valu in (0, 1):
        lib.crct_attention_force_valu(valu)
        ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=9, seed=4242)
        outs.append((ctx,) + tuple(ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=9, seed=4242)))
    lib.crct_attention_force_valu(0)
    for a, b in zip(*outs):
        assert rel_err(a, b) < 1.5e-2        # a different mask would move whole probabilities (errors of order 1)


def test_attention_dropout_statistics_and_grad_consistency(attn_path):
    B, heads, T, d, p = 16, 16, 36, 64, 0.1
    Hh = heads * d
    q, k = bf(rand(B, T, Hh, seed=1)), bf(rand(B, T, Hh, seed=2))
    v = bf(torch.ones(B, T, Hh, device=DEV))        # ctx = sum_j dropout(P)_ij  -> E = 1
    km = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=5, seed=99)
    assert abs(float(ctx.float().mean()) - 1.0) < 0.01
    assert float(ctx.float().std()) > 0.01
    # same seed -> identical; backward uses the same mask: dv = Pd^T dctx, with dctx = 1: colsum(Pd) summed = Tq
    ctx2 = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=5, seed=99)
    assert torch.equal(ctx, ctx2)
    ones = bf(torch.ones(B, T, Hh, device=DEV))
    _, _, dv = ops.attention_bwd(q, k, v, km, ones, heads, d, p_drop=p, site=5, seed=99)
    # sum_j dv[j, c] = sum_i sum_j Pd[i, j] = sum_i ctx[i, c]
    assert rel_err(dv.float().sum(1), ctx.float().sum(1)) < 1e-2


# ------------------------------------------------------------------------------------------- dropout masks against the host stream
# Every dropout site draws its bits from philox_keep8 (common.hip.h); tests/dropout_ref.py restates that stream on the host.  Each test
# below reads a kernel's mask out of its output and compares it with the host's, bit for bit, at seeds above 2^32 and at sites of the
# engine's range (1 - 3: the embeddings and cls, 16 and up: the layers).  A repeated mask, a wrong element numbering or a changed
# Philox word then fails here even though forward and backward would still agree with each other.
DROP_SEEDS = ((1 << 40) + 0x2F1D, (0x3A5 << 52) + 77)


@pytest.mark.parametrize("M,N,K", [(333, 256, 128), (21, 68, 96), (15, 132, 64), (1600, 768, 768), (7, 1028, 64)])
def test_gemm_dropout_mask_is_the_host_stream(M, N, K, gemm_path):
    """out_f32 with and without p_drop: the zeros are the mask (no output is 0 without dropout), the kept values are scaled exactly.
    M odd and N = 4 (mod 8) (the register-staged kernel only) put the 8-element groups across rows."""
    x, w = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.1, seed=2))
    y0 = ops.gemm(x, w, M, N, K, out_f32=True)
    assert bool((y0 != 0).all())
    for seed, site, p in ((DROP_SEEDS[0], 16, 0.1), (DROP_SEEDS[1], 41, 0.1), (DROP_SEEDS[0], 3, 0.5)):
        y = ops.gemm(x, w, M, N, K, out_f32=True, p_drop=p, site=site, seed=seed)
        keep = host_keep(seed, site, M, N, p)
        assert torch.equal(y != 0, keep), (seed, site, p)
        assert torch.equal(y[keep], y0[keep] * (1.0 / (1.0 - p))), (seed, site, p)


def test_gemm_fp8_dropout_mask_is_the_host_stream():
    M, N, K = 333, 256, 128
    g = torch.Generator(device="cpu").manual_seed(4)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    sa, sb = 448.0 / float(x.abs().max()), 448.0 / float(w.abs().max())
    xq, wq = _q8(x, sa).to(DEV), _q8(w, sb).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    y0 = ops.gemm_fp8(xq, wq, sa_d, sb_d, M, N, K, out_f32=True)
    assert bool((y0 != 0).all())
    for seed, site in ((DROP_SEEDS[0], 18), (DROP_SEEDS[1], 2)):
        y = ops.gemm_fp8(xq, wq, sa_d, sb_d, M, N, K, out_f32=True, p_drop=0.1, site=site, seed=seed)
        keep = host_keep(seed, site, M, N, 0.1)
        assert torch.equal(y != 0, keep), site
        assert rel_err(y[keep], y0[keep] / 0.9) < 1e-6


@pytest.mark.parametrize("M,H", [(1600, 768), (21, 64), (7, 2048), (13, 1024)])
def test_layernorm_dropout_masks_are_the_host_stream(M, H):
    """crct_layernorm_fwd (bf16 and fp32 input) and crct_layernorm_bwd: p_lin through the zeros of dx_lin, p_post through the bits of dx
    (p = 0.5 scales by exactly 2, so dropout inside the kernel and the host mask applied to dy in front of it give the same dx)."""
    x = rand(M, H, scale=2.0, seed=1) + 0.3
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3) + 0.05
    for xin in (bf(x), x):
        y0, mean, rstd = ops.layernorm_fwd(xin, gamma, beta)
        assert bool((y0 != 0).all())
        for seed, site in ((DROP_SEEDS[0], 1), (DROP_SEEDS[1], 23)):
            y, _, _ = ops.layernorm_fwd(xin, gamma, beta, p_drop=0.1, site=site, seed=seed)
            assert torch.equal(y != 0, host_keep(seed, site, M, H, 0.1)), (xin.dtype, site)
    xb = bf(x)
    _, mean, rstd = ops.layernorm_fwd(xb, gamma, beta)
    dy = bf(rand(M, H, seed=4))
    dx0, _, dg0, db0, _ = ops.layernorm_bwd(dy, xb, mean, rstd, gamma)
    assert bool((dx0 != 0).all())
    for seed, site in ((DROP_SEEDS[0], 2), (DROP_SEEDS[1], 19)):
        _, dxl, _, _, _ = ops.layernorm_bwd(dy, xb, mean, rstd, gamma, want_lin=True, p_lin=0.1, lin_site=site, seed=seed)
        assert torch.equal(dxl != 0, host_keep(seed, site, M, H, 0.1)), ("lin", site)
        keep = host_keep(seed, site, M, H, 0.5)
        dx, _, dg, db, _ = ops.layernorm_bwd(dy, xb, mean, rstd, gamma, p_post=0.5, post_site=site, seed=seed)
        dym = torch.where(keep, dy * 2, torch.zeros_like(dy))          # exact in bf16
        dx2, _, dg2, db2, _ = ops.layernorm_bwd(dym, xb, mean, rstd, gamma)
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2), ("post", site)
        # and at p = 0.1 against fp64 LayerNorm backward of dy * keep / 0.9 (the bound of test_layernorm_fwd_bwd)
        dx, *_ = ops.layernorm_bwd(dy, xb, mean, rstd, gamma, p_post=0.1, post_site=site, seed=seed)
        ks = host_keep(seed, site, M, H, 0.1).double() / 0.9
        xr = xb.double().requires_grad_(True)
        O.layer_norm(xr, gamma.double(), beta.double()).backward(dy.double() * ks)
        assert rel_err(dx, xr.grad) < 1e-2


def _attn_host_keep(seed, site, B, heads, Tq, Tk, p):
    return torch.from_numpy(DR.keep_attention(seed, site, B * heads, Tq, Tk, p)).to(DEV).view(B, heads, Tq, Tk)


def _attn_read_masks(B, heads, Tq, Tk, d, p, site, seed, row_lse=False):
    """(forward mask, backward mask), bool [B, heads, Tq, Tk], read out of the kernels: with v = identity on the key axis (in windows of d
    keys) ctx[b, i, h d + c] IS the dropped probability of key w d + c; with dctx = identity on the query axis dv[b, j, h d + c] is that of
    query w d + c.  q, k are small: every probability is far from 0."""
    Hh = heads * d
    q, k = bf(rand(B, Tq, Hh, scale=0.3, seed=1)), bf(rand(B, Tk, Hh, scale=0.3, seed=2))
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    fwd = torch.zeros(B, heads, Tq, Tk, dtype=torch.bool, device=DEV)
    bwd = torch.zeros_like(fwd)
    eye = torch.eye(d, device=DEV)
    for w0 in range(0, max(Tq, Tk), d):
        v = torch.zeros(B, Tk, heads, d, device=DEV)
        n = min(d, Tk - w0)
        if n > 0:
            v[:, w0:w0 + n] = eye[:n].view(1, n, 1, d)
        v = bf(v.view(B, Tk, Hh))
        dctx = torch.zeros(B, Tq, heads, d, device=DEV)
        nq = min(d, Tq - w0)
        if nq > 0:
            dctx[:, w0:w0 + nq] = eye[:nq].view(1, nq, 1, d)
        dctx = bf(dctx.view(B, Tq, Hh))
        lse = torch.empty(B, heads, Tq, device=DEV) if row_lse else None
        ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=site, seed=seed, row_lse=lse)
        if n > 0:
            got = ctx.view(B, Tq, heads, d)[..., :n].permute(0, 2, 1, 3)          # [B, heads, Tq, n]
            fwd[..., w0:w0 + n] = got != 0
        _, _, dv = ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=site, seed=seed, row_lse=lse,
                                     ctx=ctx if row_lse else None)
        if nq > 0:
            got = dv.view(B, Tk, heads, d)[..., :nq].permute(0, 2, 3, 1)          # [B, heads, nq, Tk]
            bwd[:, :, w0:w0 + nq] = got != 0
    return fwd, bwd


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(2, 3, 20, 36, 48), (3, 2, 7, 5, 32), (2, 2, 64, 64, 64), (2, 4, 36, 20, 32),
                                             (1, 2, 130, 130, 64), (2, 2, 40, 113, 64)])
def test_attention_dropout_masks_are_the_host_stream(B, heads, Tq, Tk, d, attn_path):
    """Forward and backward masks of every attention path (mfma / valu / long; beyond 112 keys always long, with and without kept row
    statistics) against attn_keep8's numbering on the host.  Shapes beyond 112 run the long kernels under every setting of attn_path."""
    for seed, site in ((DROP_SEEDS[0], 16), (DROP_SEEDS[1], 33)):
        want = _attn_host_keep(seed, site, B, heads, Tq, Tk, 0.1)
        for kept in ((False, True) if attn_path == "long" or max(Tq, Tk) > 112 else (False,)):
            fwd, bwd = _attn_read_masks(B, heads, Tq, Tk, d, 0.1, site, seed, row_lse=kept)
            assert torch.equal(fwd, want), (site, kept, int((fwd != want).sum()))
            assert torch.equal(bwd, want), (site, kept, int((bwd != want).sum()))


def test_attention_split_waves_draw_the_host_mask():
    """The MFMA kernels with 1, 2 and 4 waves per (batch, head) (crct_attention_force_split): each wave numbers its keys like attn_keep8."""
    lib = L.load()
    B, heads, Tq, Tk, d, seed, site = 2, 2, 64, 64, 64, DROP_SEEDS[1], 17
    want = _attn_host_keep(seed, site, B, heads, Tq, Tk, 0.1)
    try:
        for split in (1, 2, 4):
            lib.crct_attention_force_split(split)
            fwd, bwd = _attn_read_masks(B, heads, Tq, Tk, d, 0.1, site, seed)
            assert torch.equal(fwd, want) and torch.equal(bwd, want), split
    finally:
        lib.crct_attention_force_split(0)


def _attn_ref64_drop(q, k, v, km, heads, d, keep, p):
    """fp64 softmax(q k^T / sqrt(d) + mask) * keep / (1 - p) @ v (oracle.sdpa with the kernels' mask)."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh = q.view(B, Tq, heads, d).permute(0, 2, 1, 3)
    kh = k.view(B, Tk, heads, d).permute(0, 2, 1, 3)
    vh = v.view(B, Tk, heads, d).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d) + (1.0 - km.double())[:, None, None, :] * -10000.0
    pd = torch.softmax(s, -1) * keep.double() / (1.0 - p)
    return (pd @ vh).permute(0, 2, 1, 3).reshape(B, Tq, heads * d)


def _attention_fp64_under_dropout(B, heads, Tq, Tk, d, stats, km):
    Hh, p, seed, site = heads * d, 0.1, DROP_SEEDS[0] + Tq, 16 + Tk
    bufq = bf(rand(B, Tq, 3 * Hh, seed=1))
    bufk = bf(rand(B, Tk, 3 * Hh, seed=2))
    q, k, v = bufq[:, :, :Hh], bufk[:, :, Hh:2 * Hh], bufk[:, :, 2 * Hh:]
    lse = torch.empty(B, heads, Tq, device=DEV) if stats == "kept" else None
    ctx = ops.attention_fwd(q, k, v, km, heads, d, p_drop=p, site=site, seed=seed, row_lse=lse)
    keep = _attn_host_keep(seed, site, B, heads, Tq, Tk, p)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref64_drop(qr, kr, vr, km, heads, d, keep, p)
    assert rel_err(ctx, ref.detach()) < 1e-2
    dctx = bf(rand(B, Tq, Hh, seed=3))
    ref.backward(dctx.double())
    dq, dk, dv = ops.attention_bwd(q, k, v, km, dctx, heads, d, p_drop=p, site=site, seed=seed, row_lse=lse, ctx=ctx if lse is not None else None)
    assert rel_err(dq, qr.grad) < 1.5e-2
    assert rel_err(dk, kr.grad) < 1.5e-2
    assert rel_err(dv, vr.grad) < 1.5e-2


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(80, 16, 20, 20, 48), (80, 16, 36, 36, 64), (80, 32, 20, 36, 32), (80, 32, 36, 20, 32),
                                             (4, 16, 100, 100, 64), (4, 32, 40, 100, 32), (4, 32, 100, 40, 32), (3, 4, 7, 5, 16),
                                             (3, 4, 5, 7, 24), (5, 16, 64, 64, 64), (5, 8, 17, 33, 48), (2, 4, 1, 1, 32),
                                             (3, 4, 16, 48, 32), (3, 4, 49, 15, 64)])
def test_attention_fwd_bwd_under_dropout_against_fp64(B, heads, Tq, Tk, d, attn_path):
    """test_attention_fwd_bwd's shapes, key masks and bounds with p = 0.1, against fp64 autograd with the host mask."""
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    for b in range(B):
        km[b, Tk - (b % 4):] = 0
    _attention_fp64_under_dropout(B, heads, Tq, Tk, d, "recomputed", km)


@pytest.mark.parametrize("stats", ["recomputed", "kept"])
@pytest.mark.parametrize("B,heads,Tq,Tk,d", LONG_SHAPES)
def test_attention_long_sequences_under_dropout_against_fp64(B, heads, Tq, Tk, d, stats):
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    for b in range(B):
        km[b, Tk - 1 - 5 * b:] = 0
    _attention_fp64_under_dropout(B, heads, Tq, Tk, d, stats, km)


def test_gemm_epilogue_chains_under_dropout_against_fp64(gemm_path):
    """bias -> GELU -> dropout -> addend (bf16, or the fp32 residual stream) against fp64 with the host mask, at the bounds of
    test_gemm_epilogues / test_gemm_epilogue_on_the_fp32_residual_stream."""
    for M, N, K in ((333, 256, 128), (1600, 768, 768), (100, 64, 72), (21, 68, 96)):
        x, w, b = bf(rand(M, K, seed=1)), bf(rand(N, K, scale=0.1, seed=2)), rand(N, seed=3)
        r = rand(M, N, seed=4)
        seed, site = DROP_SEEDS[1] + M, 16 + N % 7
        keep = host_keep(seed, site, M, N, 0.1).double()
        u = x.double() @ w.double().t() + b.double()
        h64 = O.gelu_erf(u) * keep / 0.9
        pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        y = ops.gemm(x, w, M, N, K, bias=b, act="gelu", preact_out=pre, p_drop=0.1, site=site, seed=seed)
        assert rel_err(pre, u) < 1e-2 and rel_err(y, h64) < 1e-2, (M, N, K)
        y = ops.gemm(x, w, M, N, K, bias=b, act="gelu", p_drop=0.1, site=site, seed=seed, addend=bf(r))
        assert rel_err(y, h64 + bf(r).double()) < 1e-2, (M, N, K)
        if N % 8 == 0:
            y = ops.gemm(x, w, M, N, K, bias=b, act="gelu", p_drop=0.1, site=site, seed=seed, addend=r, out_f32=True, c_cached=True)
            assert rel_err(y, h64 + r.double()) < 2e-3, (M, N, K)
        y = ops.gemm(x, w, M, N, K, bias=b, p_drop=0.1, site=site, seed=seed, addend=r, out_f32=True)
        assert rel_err(y, u * keep / 0.9 + r.double()) < 2e-3, (M, N, K)

# ------------------------------------------------------------------------------------------- AdamW
def test_adamw_matches_torch():
    lib = L.load()
    sizes = [4096 * 3 + 17, 64, 5000, 768]
    offs, top = [], 0
    for s in sizes:
        offs.append(top)
        top += (s + 63) // 64 * 64
    g = torch.Generator().manual_seed(0)
    p = torch.randn(top, generator=g).to(DEV)
    grad = torch.randn(top, generator=g).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pb = torch.zeros(top, device=DEV, dtype=torch.bfloat16)
    lrs, wds = [2e-5, 1e-3, 2e-5, 5e-4], [0.01, 0.0, 0.01, 0.0]
    ref_params = [p[o:o + s].clone().cpu().requires_grad_(True) for o, s in zip(offs, sizes)]
    opt = torch.optim.AdamW([{"params": [rp], "lr": lr, "weight_decay": wd} for rp, lr, wd in zip(ref_params, lrs, wds)], lr=1e-3)
    blk_seg, blk_off = ops.adamw_plan(sizes)
    d = lambda t, dt: torch.as_tensor(t, dtype=dt).to(DEV)   # noqa: E731
    seg_off, seg_len, seg_lr, seg_wd = d(offs, torch.int64), d(sizes, torch.int64), d(lrs, torch.float32), d(wds, torch.float32)
    bs, bo = blk_seg.to(DEV), blk_off.to(DEV)
    for step in (1, 2, 3):
        for rp, o, s in zip(ref_params, offs, sizes):
            rp.grad = grad[o:o + s].cpu().clone() * step
        opt.step()
        L.check(lib.crct_adamw_step(p.data_ptr(), (grad * step).data_ptr(), m.data_ptr(), v.data_ptr(), pb.data_ptr(), seg_off.data_ptr(),
                                    seg_len.data_ptr(), seg_lr.data_ptr(), seg_wd.data_ptr(), bs.data_ptr(), bo.data_ptr(), bs.numel(),
                                    0.9, 0.999, 1e-8, step, None, None, None, 2 if step == 2 else 0, 0, None, L.current_stream()))   # step 2: throttled grid
    for rp, o, s in zip(ref_params, offs, sizes):
        assert torch.allclose(p[o:o + s].cpu(), rp.detach(), rtol=1e-5, atol=1e-7)
        assert torch.equal(pb[o:o + s].cpu(), p[o:o + s].cpu().to(torch.bfloat16))
    # padding between tensors is never touched
    assert float(m[sizes[0]:offs[1]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ fp8 (BASELINE configs[4])
def _q8(x, scale):
    """OCP e4m3 quantisation as the kernels do it: q = e4m3(clamp(x * scale, +-448)), round-to-nearest-even."""
    return (x.float() * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


@pytest.mark.parametrize("M,N,K", [(1600, 3072, 768), (1600, 768, 3072), (2880, 3072, 1024), (80, 256, 128)])
def test_gemm_fp8_forward(M, N, K):
    """e4m3 x e4m3 -> fp32 accumulate -> fused epilogue, against fp32 matmul of the SAME dequantised operands (the kernel's
    only freedom is the summation order and the bf16 rounding of its outputs), plus the e4m3 copy of the output."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g) * 1.5
    w = torch.randn(N, K, generator=g) * 0.05
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    sa, sb = 448.0 / float(x.abs().max()), 448.0 / float(w.abs().max())
    xq, wq = _q8(x, sa).to(DEV), _q8(w, sb).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    ref = (xq.float() / sa) @ (wq.float() / sb).t() + b
    y = ops.gemm_fp8(xq, wq, sa_d, sb_d, M, N, K, bias=b, out_f32=True)
    assert float((y - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # GELU epilogue + pre-activation + e4m3 copy of the output (what the FFN-up GEMM does)
    pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    href = torch.nn.functional.gelu(ref)
    qs = torch.tensor([448.0 / float(href.abs().max()) * 0.9], device=DEV)
    amax = torch.zeros(L.FP8_AMAX_LANES, device=DEV)      # an amax value = LANES words, the kernels spread their atomics over them
    h = ops.gemm_fp8(xq, wq, sa_d, sb_d, M, N, K, bias=b, act="gelu", preact_out=pre, q_out=q_out, q_scale=qs, q_amax=amax)
    assert float((pre.float() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    assert float((h.float() - href).abs().max()) <= 1e-2 * float(href.abs().max())
    assert abs(float(amax.max()) - float(href.abs().max())) <= 1e-2 * float(href.abs().max())
    deq = q_out.view(torch.float8_e4m3fn).float() / float(qs)
    # e4m3 keeps 3 mantissa bits: relative error <= 2^-4 of the value (plus the subnormal step near zero)
    tol = 0.0625 * href.abs() + 0.002 / float(qs) + 1e-2 * float(href.abs().max())       # + the subnormal step, + the kernel's own bf16-level differences
    assert float(((deq - href).abs() - tol).max()) <= 0.0


@pytest.mark.parametrize("M,N,K", [(1600, 3072, 768), (1600, 768, 3072), (2880, 1024, 1024), (300, 1024, 768)])
def test_gemm_fp8_data_gradient(M, N, K):
    """The fp8 BACKWARD GEMM: dx[M][N = in] = dy[M][K = out] W[out][in] as e5m2(dy) x e4m3(W^T) -- the A operand is OCP e5m2, the B
    operand the transposed e4m3 weight shadow [in][out] -- with the GELU' epilogue and an e5m2 copy of the result (what the
    FFN-down data gradient hands to the FFN-up one).  Against fp32 matmul of the same dequantised operands."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K + 1)
    dy = torch.randn(M, K, generator=g) * 3e-3
    wt = torch.randn(N, K, generator=g) * 0.05                  # = W^T: [in][out]
    u = (torch.randn(M, N, generator=g)).to(torch.bfloat16).to(DEV)
    sa, sb = 57344.0 / float(dy.abs().max()), 448.0 / float(wt.abs().max())
    dyq = (dy * sa).clamp(-57344, 57344).to(torch.float8_e5m2).to(DEV)
    wq = _q8(wt, sb).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    ref = (dyq.float() / sa) @ (wq.float() / sb).t()
    dx = ops.gemm_fp8(dyq, wq, sa_d, sb_d, M, N, K, out_f32=True, a_bf8=True)
    assert float((dx - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # x gelu'(u), e5m2 copy of the result + its amax
    uf = u.float()
    gprime = 0.5 * (1 + torch.erf(uf / math.sqrt(2))) + uf * torch.exp(-0.5 * uf * uf) / math.sqrt(2 * math.pi)
    ref2 = ref * gprime
    q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    qs = torch.tensor([57344.0 / float(ref2.abs().max()) * 0.5], device=DEV)
    amax = torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    du = ops.gemm_fp8(dyq, wq, sa_d, sb_d, M, N, K, a_bf8=True, q_bf8=True, dact_src=u, dact="gelu", q_out=q_out, q_scale=qs, q_amax=amax)
    assert float((du.float() - ref2).abs().max()) <= 1e-2 * float(ref2.abs().max())
    assert abs(float(amax.max()) - float(ref2.abs().max())) <= 1e-2 * float(ref2.abs().max())
    deq = q_out.view(torch.float8_e5m2).float() / float(qs)
    tol = 0.125 * ref2.abs() + 1e-2 * float(ref2.abs().max())          # e5m2: 2 mantissa bits -> half an ulp = 2^-3 relative
    assert float(((deq - ref2).abs() - tol).max()) <= 0.0


@pytest.mark.parametrize("R,N,K", [(1600, 3072, 768), (1600, 768, 3072), (2880, 1024, 1024), (80, 1024, 1024), (1, 64, 48), (257, 208, 80), (768, 768, 1024)])
def test_gemm_fp8_weight_gradient(R, N, K):
    """The fp8 WEIGHT-GRADIENT GEMM: dW[N = out][K = in] = dy^T x from the token-major copies the other passes left behind --
    dy [R tokens][out] OCP e5m2, x [R][in] e4m3 -- read through the transposing LDS load; R is the contraction length (any
    value: the tail of the last 128-token tile is zero-filled), N / K need not fill a tile.  Against fp32 matmul of the same
    dequantised operands: overwrite, accumulate onto an existing gradient, and the identity check with an ASYMMETRIC x that
    catches a transposed result (cdna_hip_programming.md section 3)."""
    g = torch.Generator(device="cpu").manual_seed(R + N + K + 3)
    dy = torch.randn(R, N, generator=g) * 3e-3
    x = torch.randn(R, K, generator=g)
    s_dy, s_x = 57344.0 / float(dy.abs().max()), 448.0 / float(x.abs().max())
    dyq = (dy * s_dy).clamp(-57344, 57344).to(torch.float8_e5m2).to(DEV)
    xq = _q8(x, s_x).to(DEV)
    sd, sx = torch.tensor([s_dy], device=DEV), torch.tensor([s_x], device=DEV)
    ref = (dyq.float() / s_dy).t() @ (xq.float() / s_x)
    bound = 2e-3 * float(ref.abs().max()) + 1e-9
    for tile in (36, 37):
        out = torch.full((N, K), 7.0, device=DEV)
        ops.gemm_wgrad_fp8([(dyq, xq, sd, sx, out)], accumulate=False, tile=tile)
        assert float((out - ref).abs().max()) <= bound, tile
        ops.gemm_wgrad_fp8([(dyq, xq, sd, sx, out)], accumulate=True, tile=tile)
        assert float((out - 2 * ref).abs().max()) <= 2 * bound, tile
    if R == N:           # dy = identity: dW must be x itself (quantised), not its transpose
        eye = torch.eye(R).to(torch.float8_e5m2).to(DEV)
        one = torch.ones(1, device=DEV)
        out = torch.zeros(N, K, device=DEV)
        ops.gemm_wgrad_fp8([(eye, xq, one, sx, out)], accumulate=False)
        assert torch.equal(out, xq.float() / s_x)


def test_gemm_fp8_weight_gradients_grouped():
    """The fp8 weight gradients of a text layer in ONE launch (FFN-up, FFN-down, attention output, QKV), bit-identical to the
    single launches."""
    R = 1600
    shapes = [(3072, 768), (768, 3072), (768, 768), (2304, 768)]
    g = torch.Generator(device="cpu").manual_seed(9)
    probs, singles = [], []
    for N, K in shapes:
        dy, x = torch.randn(R, N, generator=g) * 2e-3, torch.randn(R, K, generator=g)
        s_dy, s_x = 57344.0 / float(dy.abs().max()), 448.0 / float(x.abs().max())
        dyq, xq = (dy * s_dy).to(torch.float8_e5m2).to(DEV), _q8(x, s_x).to(DEV)
        sd, sx = torch.tensor([s_dy], device=DEV), torch.tensor([s_x], device=DEV)
        probs.append((dyq, xq, sd, sx, torch.zeros(N, K, device=DEV)))
        singles.append((dyq, xq, sd, sx, torch.zeros(N, K, device=DEV)))
    ops.gemm_wgrad_fp8(probs, accumulate=False)
    for p in singles:
        ops.gemm_wgrad_fp8([p], accumulate=False)
    for a, b in zip(probs, singles):
        assert torch.equal(a[4], b[4])
        ref = (a[0].float() / float(a[2])).t() @ (a[1].float() / float(a[3]))
        assert float((a[4] - ref).abs().max()) <= 2e-3 * float(ref.abs().max())


def test_layernorm_bwd_emits_the_e5m2_gradient_copy():
    """CrctLnBwdArgs.q_out: the gradient that leaves the LayerNorm-backward kernel towards the producing Linear, also as OCP e5m2
    (the A operand of that Linear's fp8 data gradient), quantised from the bf16-rounded value; its maximum in q_amax."""
    lib = L.load()
    M, H = 1600, 768
    dy, x = bf(rand(M, H, scale=2e-3, seed=1)), bf(rand(M, H, seed=2))
    gamma = rand(H, seed=3)
    mean, rstd = x.float().mean(1), 1.0 / torch.sqrt(x.float().var(1, unbiased=False) + 1e-12)
    dx_ref, dxl_ref, _, _, _ = ops.layernorm_bwd(dy, x, mean, rstd, gamma, want_lin=True, p_lin=0.1, lin_site=7, seed=5)
    a = L.LnBwdArgs()
    dx, dxl = torch.empty_like(x), torch.empty_like(x)
    nb = lib.crct_layernorm_bwd_blocks(M)
    part = torch.empty(3 * 4 * nb * H, device=DEV)
    q = torch.zeros(M, H, dtype=torch.uint8, device=DEV)
    qs, am = torch.tensor([4096.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    a.dy, a.x, a.mean, a.rstd, a.gamma, a.dx, a.dx_lin, a.partials = (L.ptr(t) for t in (dy, x, mean, rstd, gamma, dx, dxl, part))
    a.M, a.H, a.post_thr, a.post_scale, a.post_site = M, H, 0, 1.0, 0
    a.lin_thr, a.lin_scale, a.lin_site, a.seed = L.drop_threshold(0.1), 1.0 / 0.9, 7, 5
    a.q_out, a.q_scale, a.q_amax = L.ptr(q), L.ptr(qs), L.ptr(am)
    L.check(lib.crct_layernorm_bwd_rows_args(C.byref(a), L.current_stream()), "layernorm_bwd_rows_args")
    assert torch.equal(dx, dx_ref) and torch.equal(dxl, dxl_ref)
    want = (dxl_ref.float() * 4096.0).clamp(-57344, 57344).to(torch.float8_e5m2)
    assert torch.equal(q.view(torch.float8_e5m2).float(), want.float())
    assert float(am.max()) == float(dxl_ref.float().abs().max())


def test_fp8_quantisers_and_layernorm_copy():
    lib = L.load()
    # bf16 -> e4m3 pass
    x = (torch.randn(1600 * 768, device=DEV) * 2).to(torch.bfloat16)
    q = torch.zeros(x.numel(), device=DEV, dtype=torch.uint8)
    sc, am = torch.tensor([17.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    L.check(lib.crct_fp8_quantize_bf16(x.data_ptr(), q.data_ptr(), sc.data_ptr(), am.data_ptr(), x.numel(), L.current_stream()))
    assert torch.equal(q.view(torch.float8_e4m3fn).float(), _q8(x, 17.0).float())
    assert float(am.max()) == float(x.float().abs().max())
    # skip_if != 0 (GradScaler's found_inf): the call must leave scale AND amax untouched
    skip = torch.ones(1, device=DEV)
    L.check(lib.crct_fp8_update_scales(sc.data_ptr(), am.data_ptr(), 1, 1, skip.data_ptr(), 448.0, L.current_stream()))
    assert float(sc) == 17.0 and float(am.max()) == float(x.float().abs().max())
    skip.zero_()
    L.check(lib.crct_fp8_update_scales(sc.data_ptr(), am.data_ptr(), 1, 1, skip.data_ptr(), 448.0, L.current_stream()))
    assert abs(float(sc) - 448.0 / float(x.float().abs().max())) < 1e-4 * float(sc) and float(am.abs().max()) == 0.0
    # LayerNorm with the e4m3 copy: the copy is the quantisation of the bf16 output the kernel stores
    xs = (torch.randn(1600, 768, device=DEV)).to(torch.bfloat16)
    gamma, beta = torch.rand(768, device=DEV) + 0.5, torch.randn(768, device=DEV) * 0.1
    y = torch.empty_like(xs)
    mean, rstd = torch.empty(1600, device=DEV), torch.empty(1600, device=DEV)
    yq = torch.zeros(1600, 768, device=DEV, dtype=torch.uint8)
    sc2, am2 = torch.tensor([30.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    L.check(lib.crct_layernorm_fwd_q(xs.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                     1600, 768, 1e-12, 0, 1.0, 0, 0, yq.data_ptr(), sc2.data_ptr(), am2.data_ptr(), L.current_stream()))
    y_plain, _, _ = ops.layernorm_fwd(xs, gamma, beta)
    assert torch.equal(y, y_plain)
    assert torch.equal(yq.view(torch.float8_e4m3fn).float(), _q8(y, 30.0).float())
    assert float(am2.max()) == float(y.float().abs().max())


# ------------------------------------------------------------------------------------------- embeddings against fp64
# The kernels at the front of the step (rowops.hip: crct_embed_text_* / crct_embed_image_*) against plain fp64 restatements on the CPU.
# Forward: the saved pre-norm sum, y and the row statistics element by element.  Backward: every gradient output per element against
# fp64 autograd fed the kernel's own saved sum (the LayerNorm backward is taken where the kernel takes it), bound
#   |got - ref| <= 1e-4 * sum|contributions| + 1e-6
# where the sum runs over the pre-filled value and every per-token term that reaches the element (a per-tensor norm would hide one
# missing row of one id).

def _bf16_step(x):
    """Spacing of the bf16 numbers at |x| (fp64): 2^(exponent - 7); the smallest normal's below it."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _assert_within_bf16_step(got, ref, scale, what):
    """|got - ref| <= one bf16 step at max(|got|, |ref|) + 2^-20 * scale.  scale = the magnitude of the fp32 terms the kernel combined before
    rounding to bf16: their own fp32 roundings may move a result that sits at a rounding boundary, or one that cancels, by that much
    (2^-20 is 1/8192 of a bf16 step at the same magnitude)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    tol = _bf16_step(torch.maximum(got.abs(), ref.abs())) + 2.0 ** -20 * scale
    bad = err > tol
    assert not bool(bad.any()), "%s: %d elements beyond one bf16 step, first at %s (got %r, fp64 %r)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]))


def _assert_sums(got, ref, mag, what):
    """Per element: |got - ref| <= 1e-4 * mag + 1e-6, mag = sum of |contributions| (the pre-filled value included)."""
    err = (got.double().cpu() - ref).abs()
    bad = err > 1e-4 * mag + 1e-6
    assert not bool(bad.any()), "%s: %d elements off, first at %s (got %r, fp64 %r, sum|terms| %r)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got.double().cpu()[bad][0]), float(ref[bad][0]),
        float(mag[bad][0]))


def _ln_stats64(x):
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, var.sqrt(), 1.0 / torch.sqrt(var + O.LN_EPS)


def _check_ln_forward(sum_b, y, mean, rstd, gamma, beta, p, site, seed, what):
    """mean / rstd against fp64 statistics of the saved (bf16) sum, y against fp64 LayerNorm of it (kept elements / (1 - p) under
    dropout, dropped ones exactly 0) -- and, under dropout, against crct_layernorm_fwd of the saved sum with the same (site, seed)."""
    x = sum_b.double().cpu()
    m64, sd64, r64 = _ln_stats64(x)
    assert float(((mean.double().cpu() - m64).abs() / (m64.abs() + sd64)).max()) <= 1e-5, what + ": mean"
    assert float(((rstd.double().cpu() - r64).abs() / r64).max()) <= 1e-5, what + ": rstd"
    g, b = gamma.double().cpu(), beta.double().cpu()
    xn = (x - m64[:, None]) * r64[:, None]
    ref = g * xn + b
    scale = (g * xn).abs() + b.abs()
    yc = y.cpu()
    if p == 0.0:
        _assert_within_bf16_step(yc, ref, scale, what + ": y")
        return torch.ones_like(ref)
    # The embedding kernels and crct_layernorm_fwd both normalise through row_stats / row_normalize on the same bf16 values of the same row
    # index with the same (site, seed): the same mask and the same bits.
    y_ln, _, _ = ops.layernorm_fwd(sum_b, gamma, beta, p_drop=p, site=site, seed=seed)
    keep = yc != 0
    assert torch.equal(keep, y_ln.cpu() != 0), what + ": dropout mask differs from crct_layernorm_fwd's"
    assert torch.equal(keep, host_keep(seed, site, *y.shape, p).cpu()), what + ": dropout mask differs from the host Philox stream's"
    if keep.numel() > 20000:
        assert abs(float(keep.double().mean()) - (1 - p)) < 0.02, what + ": dropout rate"
    _assert_within_bf16_step(yc[keep], ref[keep] / (1 - p), scale[keep] / (1 - p), what + ": kept y")
    assert torch.equal(y, y_ln), what + ": y differs from crct_layernorm_fwd of the saved sum"
    return keep.double() / (1 - p)


def _ln_backward64(sum_b, dy, keep_scale, gamma):
    """fp64 autograd of LayerNorm at the saved sum, fed dy * keep / (1 - p): (d_sum, d_gamma, d_beta, |dy'| * |xhat|, |dy'|)."""
    x = sum_b.double().cpu().requires_grad_(True)
    g = gamma.double().cpu().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    dyv = dy.double().cpu() * keep_scale
    O.layer_norm(x, g, b).backward(dyv)
    m64, _, r64 = _ln_stats64(x.detach())
    xn = (x.detach() - m64[:, None]) * r64[:, None]
    return x.grad, g.grad, b.grad, (dyv * xn).abs().sum(0), dyv.abs().sum(0)


_TEXT_V, _TEXT_NPOS, _TEXT_NTYPES = 4099, 512, 5
# (B, T) -> (H, dropout p): configs[1]; the test's original small shapes; plotqa-real; one token; the NCH 1 and NCH 4 row widths; positions
# up to 511; 14 336 rows (the word-table sums above 64 KiB of LDS); 16 384 rows > GATHER_MAX_ROWS (every table sum through float atomics)
_TEXT_CASES = {(80, 20): (768, 0.1), (7, 9): (768, 0.0), (64, 40): (768, 0.0), (80, 124): (768, 0.1), (1, 1): (768, 0.0),
               (3, 7): (64, 0.1), (2, 9): (2048, 0.1), (1, 512): (768, 0.0), (112, 128): (768, 0.1), (32, 512): (768, 0.1)}
_GATHER_MAX_ROWS = 15360      # rowops.hip: above it the table sums fall back to float atomics


def _text_batch(B, T, seed):
    """ids / segments / loc crafted for the gates and the word-gradient sums' edge cases: [PAD]-like id 0 on half of all rows (hundreds of
    matches: the heavy path), [CLS]-like id 1 once per batch row, four heavy ids (9 / 15 / 16 / 17 matches) whose first rows fill one 4-row
    workgroup, an id whose matches straddle a 64-row and a 256-row window (light, and heavy), ids with exactly 1, 2, 3, 8, 9, 11, 15, 16 and
    17 matches, id V - 1, an id that first occurs in the last row; segments -1 / 0 / 1 / 2.. n_types - 1 with batch rows without a
    question / answer token and rows whose first one sits mid-row; all-zero loc rows, rows with one non-zero coordinate, rows whose
    coordinates sum to 0."""
    M, V = B * T, _TEXT_V
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(24, V - 1, (M,), generator=g)            # filler: ids 24 .. V-2, one to a few matches each
    ids.view(B, T)[:, T // 2:] = 0
    ids.view(B, T)[:, 0] = 1
    free = [r for r in range(M) if 0 < r % T < T // 2]
    taken = set()

    def put(i, rows):
        for r in rows:
            assert r not in taken
            taken.add(r)
            ids[r] = i

    def rest(after=-1):
        return [r for r in free if r not in taken and r > after]

    # four heavy ids whose first rows are the four rows of one workgroup
    grp = next((r for r in free if r % 4 == 0 and all(r + k in free for k in range(4))), None)
    if grp is not None and len(rest(grp + 3)) >= 9 + 15 + 16 + 17 - 4:
        for k, n in enumerate((9, 15, 16, 17)):
            later = rest(grp + 3)
            pick = sorted(later[int(j)] for j in torch.randperm(len(later), generator=g)[:n - 1])
            put(2 + k, [grp + k] + pick)
    # matches across the 64-row and the 256-row windows of the scans: first row just below 64, then 64 and beyond, then beyond the first
    # 256-row window of the indexed scan ((r + 1) & ~63 .. + 255)
    lo = [r for r in rest() if r < 64]
    if lo and len(rest(lo[-1] + 256)) >= 14:
        r0 = lo[-1]
        a = rest(r0)
        b = rest(((r0 + 1) & ~63) + 255)
        put(6, [r0, a[0], a[1], b[0], b[1]])                       # 5 matches: the light path
        lo = [r for r in rest() if r < 64]
        r1 = lo[-1]
        far = rest(((r1 + 1) & ~63) + 255)
        near = rest(r1)[:3]
        put(7, [r1] + near + far[:8])                               # 12 matches: the heavy path
    for i, n in zip(range(8, 17), (1, 2, 3, 8, 9, 11, 15, 16, 17)):
        avail = rest()
        if len(avail) < n + 2:
            break
        put(i, sorted(avail[int(j)] for j in torch.randperm(len(avail), generator=g)[:n]))
    avail = rest()
    if len(avail) >= 2:
        put(V - 1, avail[-2:])
    if M > 1:
        ids[M - 1] = 23                                              # first (and only) occurrence in the last row
    else:
        ids[0] = V - 1
    # segments: row kind (b + 2) % 4 -- 2, 3: a QA token at t = 0 and at t = T - 1 (positions up to T - 1); 0: no QA token; 1: the first
    # QA token at T // 3
    segs = torch.randint(-1, _TEXT_NTYPES, (B, T), generator=g)
    for b in range(B):
        kind = (b + 2) % 4
        row = segs[b]
        no_qa = torch.tensor([0, 2, 3, 4])[torch.randint(0, 4, (T,), generator=g)]
        if kind == 0:
            row.copy_(no_qa)
        elif kind == 1:
            row[:T // 3] = no_qa[:T // 3]
            row[T // 3] = -1
        else:
            row[0], row[T - 1] = 1, -1 if T > 1 else 1
    loc = torch.rand(M, 4, generator=g) * 2 - 1
    r = torch.arange(M)
    loc[r % 5 == 0] = 0.0
    one = r % 5 == 1
    keepc = torch.nn.functional.one_hot((r // 5) % 4, 4).bool()
    loc[one] = torch.where(keepc[one], loc[one], torch.zeros(()))
    zs = r % 7 == 3
    loc[zs] = torch.tensor([0.7, -0.7, 0.0, 0.0])                  # sums to 0: the gate is on |loc|_1
    return ids.view(B, T), segs, loc.view(B, T, 4)


def _text_terms(tab, ids, segs, loc):
    """vilbert.py:320-354 in fp64 (oracle.embed_text without its LayerNorm and dropout): the pre-norm sum as a function of the tables."""
    B, T = ids.shape
    not_qa = (segs != -1) & (segs != 1)
    pos = torch.arange(T).unsqueeze(0).expand(B, T).clone()
    pos[not_qa] = T
    pos = pos - pos.min(dim=-1)[0].unsqueeze(1)
    pos[not_qa] = 0
    tt = segs.clone()
    tt[tt == -1] = 0
    loc_e = (loc @ tab["w_loc"].t() + tab["b_loc"]) * (loc.abs().sum(-1) != 0).unsqueeze(-1)
    return (tab["word"][ids] + tab["pos"][pos] * (~not_qa).unsqueeze(-1) + tab["type"][tt] * (segs != 0).unsqueeze(-1)
            + loc_e).reshape(B * T, -1)


@pytest.mark.parametrize("B,T", list(_TEXT_CASES))
def test_word_gradient_indexed_split_and_atomic_forms_agree_and_are_reproducible(B, T, gemm_path):
    """crct_embed_text_fwd / _bwd_indexed (BertEmbeddingLocation.forward, vilbert.py:320-358) against fp64, in every form of the backward:
    indexed (the step engine's call), the two-launch test form and the float-atomics fall-back (rows_scratch = NULL).  The word_embeddings
    gradient is the index_add of the token-row gradients (vilbert.py:300 has no padding_idx, so [PAD] collects every padded position); the
    fixed-order forms -- light ids by one wave, heavy ids shared by the workgroup -- give the same bits as each other and when repeated, and
    the float atomics the same sums to rounding."""
    # no GEMM here: the test runs under both settings of the GEMM-path switch (gemm_path), which must not reach these kernels
    lib = L.load()
    H, p = _TEXT_CASES[(B, T)]
    V, n_pos, n_types = _TEXT_V, _TEXT_NPOS, _TEXT_NTYPES
    M = B * T
    site, seed = 1, (1 << 40) + 0x5EED + B              # the text embedding's site, a seed above 2^32 (the model's reach 2^62)
    ids_c, segs_c, loc_c = _text_batch(B, T, seed=B * 100 + T)
    ids, segs, loc = ids_c.to(DEV), segs_c.to(DEV), loc_c.contiguous().to(DEV)
    tab = dict(word=rand(V, H, scale=0.5, seed=11), pos=rand(n_pos, H, scale=0.5, seed=12), type=rand(n_types, H, scale=0.5, seed=13),
               w_loc=rand(H, 4, scale=0.5, seed=14), b_loc=rand(H, scale=0.5, seed=15))
    gamma, beta = 1 + 0.1 * rand(H, seed=16), 0.1 * rand(H, seed=17)
    stream = L.current_stream()
    thr, sc, st = ops._drop(p, site)

    # forward
    sum_b, y = (torch.empty(M, H, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    L.check(lib.crct_embed_text_fwd(ids.data_ptr(), segs.data_ptr(), loc.data_ptr(), tab["word"].data_ptr(), tab["pos"].data_ptr(),
                                    tab["type"].data_ptr(), tab["w_loc"].data_ptr(), tab["b_loc"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                    sum_b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, T, H, n_pos, 1e-12, thr, sc, st, seed,
                                    stream), "embed_text_fwd")
    torch.cuda.synchronize()
    t64 = {k: v.double().cpu().requires_grad_(True) for k, v in tab.items()}
    ids64, segs64, loc64 = ids_c, segs_c, loc_c.double()
    s64 = _text_terms(t64, ids64, segs64, loc64)
    s_abs = _text_terms({k: v.detach().abs() for k, v in t64.items()}, ids64, segs64, loc64.abs())
    # the restatement is the oracle's embedding up to its LayerNorm
    import types
    ref_e = O.embed_text({"bert.embeddings." + k: v.detach() for k, v in dict(
        [("word_embeddings.weight", t64["word"]), ("position_embeddings.weight", t64["pos"]), ("plotqa_type_embeddings.weight", t64["type"]),
         ("txt_location_embeddings.weight", t64["w_loc"]), ("txt_location_embeddings.bias", t64["b_loc"]),
         ("LayerNorm.weight", gamma.double().cpu()), ("LayerNorm.bias", beta.double().cpu())]).items()},
        types.SimpleNamespace(hidden_dropout_prob=p), ids64, segs64, loc64, training=False)
    assert float((ref_e.reshape(M, H) - O.layer_norm(s64.detach(), gamma.double().cpu(), beta.double().cpu())).abs().max()) < 1e-9
    _assert_within_bf16_step(sum_b, s64.detach(), s_abs, "text sum")
    keep_scale = _check_ln_forward(sum_b, y, mean, rstd, gamma, beta, p, site, seed, "text")

    # fp64 backward: LayerNorm at the saved sum, then the (linear) restatement's table gradients
    dy = bf(rand(M, H, seed=1))
    ds, dg64, db64, dg_mag, db_mag = _ln_backward64(sum_b, dy, keep_scale, gamma)
    names = ("word", "pos", "type", "w_loc", "b_loc")
    refs = torch.autograd.grad(s64, [t64[k] for k in names], ds)
    # sum |terms|: the same linear map applied to |d_sum| with |loc| (every coefficient then non-negative)
    t_abs = {k: v.detach().abs().requires_grad_(True) for k, v in t64.items()}
    mags = torch.autograd.grad(_text_terms(t_abs, ids64, segs64, loc64.abs()), [t_abs[k] for k in names], ds.abs())
    shapes = dict(word=(V, H), pos=(n_pos, H), type=(n_types, H), w_loc=(H, 4), b_loc=(H,), gamma=(H,), beta=(H,))
    pre = {k: rand(*s, seed=40 + i) for i, (k, s) in enumerate(shapes.items())}      # outputs are accumulated into
    ref = {k: pre[k].double().cpu() + r for k, r in zip(names, refs)}
    ref.update(gamma=pre["gamma"].double().cpu() + dg64, beta=pre["beta"].double().cpu() + db64)
    mag = {k: pre[k].double().cpu().abs() + m for k, m in zip(names, mags)}
    mag.update(gamma=pre["gamma"].double().cpu().abs() + dg_mag, beta=pre["beta"].double().cpu().abs() + db_mag)
    touched = {k: m.cpu() != pre[k].double().cpu().abs() for k, m in mag.items()}

    index = torch.zeros(2 * V, dtype=torch.int32, device=DEV)
    nblk = lib.crct_layernorm_bwd_blocks(M)

    def run(mode):
        out = {k: v.clone() for k, v in pre.items()}
        partials = torch.empty(9 * 4 * nblk * H, device=DEV)
        rows = torch.empty(M, H, device=DEV) if mode != "atomic" else None
        idx = torch.empty(2 * M, dtype=torch.int32, device=DEV)
        a = [dy.data_ptr(), sum_b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ids.data_ptr(), segs.data_ptr(), loc.data_ptr(),
             gamma.data_ptr()] + [out[k].data_ptr() for k in ("word", "pos", "type", "w_loc", "b_loc", "gamma", "beta")] + [
            partials.data_ptr(), B, T, H, n_pos, thr, sc, st, seed, L.ptr(rows), idx.data_ptr(), n_types]
        if mode == "split":
            lib.crct_embed_scatter_split(1)
        try:      # first / last row per id left by the row kernel
            rc = lib.crct_embed_text_bwd_indexed(*a, index.data_ptr(), V, stream)
        finally:
            lib.crct_embed_scatter_split(0)
        L.check(rc, "embed_text_bwd " + mode)
        torch.cuda.synchronize()
        assert int(index.abs().max()) == 0      # the index is all zero again after every call
        return {k: v.cpu() for k, v in out.items()}

    got = {m: run(m) for m in ("indexed", "split", "atomic")}
    for m, o in got.items():
        for k in shapes:
            _assert_sums(o[k], ref[k], mag[k], "%s d_%s" % (m, k))
            untouched = ~touched[k]
            assert torch.equal(o[k][untouched], pre[k].cpu()[untouched]), "%s d_%s: a row no token reaches changed" % (m, k)
    w1 = got["indexed"]["word"]
    assert float((w1[0] - pre["word"][0].cpu()).abs().max()) > 0 or M == 1
    if M <= _GATHER_MAX_ROWS:
        # the fixed-order forms: the same bits as each other (one launch or two) and when repeated
        again = run("indexed")
        for k in shapes:
            assert torch.equal(got["indexed"][k], again[k]), k
            assert torch.equal(got["indexed"][k], got["split"][k]), k
    # ... and the float atomics: the same sums up to their arrival-order rounding
    for k in ("word", "pos", "type"):
        a, b = got["indexed"][k], got["atomic"][k]
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-6, k


_IMG_NCOLOR = 229      # categories + 1 (PlotQA: 228)
# (M, H, dropout p): configs[1] (80 x 36), plotqa-real (80 x 44), configs[3] (64 x 100), one element, NCH 1, NCH 4, 16 000 rows >
# GATHER_MAX_ROWS (the colour sums through float atomics)
_IMG_CASES = [(2880, 1024, 0.1), (3520, 1024, 0.0), (6400, 1024, 0.1), (1, 1024, 0.0), (7, 64, 0.1), (5, 2048, 0.0), (16000, 1024, 0.1)]


@pytest.mark.parametrize("M,H,p", _IMG_CASES)
def test_image_embedding_against_fp64(M, H, p, gemm_path):
    """crct_embed_image_fwd / _bwd (BertImageEmbeddings.forward, dataset 'plotqa', vilbert.py:1474-1496) against fp64: the saved sum, y and
    the row statistics; d_sum within one bf16 rounding; the colour-table, loc-Linear, image-Linear-bias and LayerNorm gradients per element,
    accumulated onto pre-filled outputs, through the fixed-order gather and through the float atomics."""
    lib = L.load()
    n_color, site, seed = _IMG_NCOLOR, 2, (3 << 60) + 0xC0FFEE + M     # the image embedding's site
    g = torch.Generator().manual_seed(M + H)
    target = torch.randint(0, n_color, (M,), generator=g)
    target[: M // 3] = 17                                            # one heavily repeated colour
    target[-1] = 0
    if M > 1:
        target[M // 2] = n_color - 1                                 # 0 and `categories`, the last row of the table
    loc = torch.rand(M, 4, generator=g)
    img = bf(rand(M, H, scale=0.5, seed=21))                         # new_image_embeddings(softmax(feat)) as the GEMM leaves it (bf16)
    tab = dict(color=rand(n_color, H, scale=0.5, seed=22), w_loc=rand(H, 4, scale=0.5, seed=23), b_loc=rand(H, scale=0.5, seed=24))
    gamma, beta = 1 + 0.1 * rand(H, seed=25), 0.1 * rand(H, seed=26)
    target_d, loc_d = target.to(DEV), loc.to(DEV)
    stream = L.current_stream()
    thr, sc, st = ops._drop(p, site)
    sum_b, y = (torch.empty(M, H, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    L.check(lib.crct_embed_image_fwd(img.data_ptr(), loc_d.data_ptr(), target_d.data_ptr(), tab["w_loc"].data_ptr(), tab["b_loc"].data_ptr(),
                                     tab["color"].data_ptr(), gamma.data_ptr(), beta.data_ptr(), sum_b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), M, H, 1e-12, thr, sc, st, seed, stream), "embed_image_fwd")
    torch.cuda.synchronize()
    # vilbert.py:1478-1486 in fp64 (oracle.embed_image after its feature Linear, before its LayerNorm)
    t64 = {k: v.double().cpu().requires_grad_(True) for k, v in tab.items()}
    img64, loc64 = img.double().cpu(), loc.double()
    s64 = img64 + loc64 @ t64["w_loc"].t() + t64["b_loc"] + t64["color"][target]
    s_abs = img64.abs() + loc64 @ t64["w_loc"].detach().abs().t() + t64["b_loc"].detach().abs() + t64["color"].detach().abs()[target]
    _assert_within_bf16_step(sum_b, s64.detach(), s_abs, "image sum")
    keep_scale = _check_ln_forward(sum_b, y, mean, rstd, gamma, beta, p, site, seed, "image")

    dy = bf(rand(M, H, seed=2))
    ds, dg64, db64, dg_mag, db_mag = _ln_backward64(sum_b, dy, keep_scale, gamma)
    names = ("color", "w_loc", "b_loc")
    refs = torch.autograd.grad(s64, [t64[k] for k in names], ds)
    t_abs = {k: v.detach().abs().requires_grad_(True) for k, v in t64.items()}
    mags = torch.autograd.grad(loc64 @ t_abs["w_loc"].t() + t_abs["b_loc"] + t_abs["color"][target], [t_abs[k] for k in names], ds.abs())
    shapes = dict(color=(n_color, H), w_loc=(H, 4), b_loc=(H,), b_img=(H,), gamma=(H,), beta=(H,))
    pre = {k: rand(*s, seed=60 + i) for i, (k, s) in enumerate(shapes.items())}
    ref = {k: pre[k].double().cpu() + r for k, r in zip(names, refs)}
    mag = {k: pre[k].double().cpu().abs() + m for k, m in zip(names, mags)}
    ref.update(b_img=pre["b_img"].double().cpu() + ds.sum(0), gamma=pre["gamma"].double().cpu() + dg64, beta=pre["beta"].double().cpu() + db64)
    mag.update(b_img=pre["b_img"].double().cpu().abs() + ds.abs().sum(0), gamma=pre["gamma"].double().cpu().abs() + dg_mag,
               beta=pre["beta"].double().cpu().abs() + db_mag)
    # d_sum: the fp32 row gradient rounded to bf16 once; its fp32 terms are rstd * (|g dy'| + mean|g dy'| + |xhat| mean|g dy' xhat|) -- the two
    # row means are fp32 sums over H terms, whose rounding goes with the terms' magnitude, not the mean's (a dropped element's d_sum is
    # nothing but those means)
    x = sum_b.double().cpu()
    m64, _, r64 = _ln_stats64(x)
    xn = (x - m64[:, None]) * r64[:, None]
    gd = dy.double().cpu() * keep_scale * gamma.double().cpu()
    ds_scale = r64[:, None] * (gd.abs() + gd.abs().mean(-1, keepdim=True) + xn.abs() * (gd * xn).abs().mean(-1, keepdim=True))
    nblk = lib.crct_layernorm_bwd_blocks(M)

    def run(mode):
        out = {k: v.clone() for k, v in pre.items()}
        d_sum = torch.empty(M, H, device=DEV, dtype=torch.bfloat16)
        partials = torch.empty(7 * 4 * nblk * H, device=DEV)
        rows = torch.empty(M, H, device=DEV) if mode == "gather" else None
        idx = torch.empty(M, dtype=torch.int32, device=DEV)
        L.check(lib.crct_embed_image_bwd(dy.data_ptr(), sum_b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), loc_d.data_ptr(), target_d.data_ptr(),
                                         gamma.data_ptr(), d_sum.data_ptr(), out["color"].data_ptr(), out["w_loc"].data_ptr(), out["b_loc"].data_ptr(),
                                         out["b_img"].data_ptr(), out["gamma"].data_ptr(), out["beta"].data_ptr(), partials.data_ptr(), M, H,
                                         thr, sc, st, seed, L.ptr(rows), idx.data_ptr(), n_color, stream), "embed_image_bwd " + mode)
        torch.cuda.synchronize()
        return d_sum.cpu(), {k: v.cpu() for k, v in out.items()}

    res = {m: run(m) for m in ("gather", "atomic")}
    used = torch.zeros(n_color, dtype=torch.bool)
    used[target] = True
    for m, (d_sum, o) in res.items():
        _assert_within_bf16_step(d_sum, ds, ds_scale, "%s d_sum" % m)
        for k in shapes:
            _assert_sums(o[k], ref[k], mag[k], "%s d_%s" % (m, k))
        assert torch.equal(o["color"][~used], pre["color"].cpu()[~used]), m
    assert torch.equal(res["gather"][0], res["atomic"][0])
    if M <= _GATHER_MAX_ROWS:
        d2, o2 = run("gather")
        assert torch.equal(d2, res["gather"][0]) and all(torch.equal(o2[k], res["gather"][1][k]) for k in shapes)


# ------------------------------------------------------------------------------------------- key masks
@pytest.mark.parametrize("B,T,V,S", [(5, 20, 9, 6), (3, 7, 40, 4), (80, 124, 44, 9), (1, 1, 1, 1)])
def test_build_keymasks_against_the_oracle_masks(B, T, V, S):
    """crct_build_keymasks against oracle.text_key_mask (encoder_decorator.py:118-120) and image_mask != 0: hist_len at 0 and at sep_stride - 1,
    sep_indices + 1 at 0 and at or beyond T, image_mask values other than 0 and 1, T > V and V > T (the grid covers the larger one), and
    each mask alone (NULL for the other).  Every output byte starts as 0xAB: each one must be written."""
    lib = L.load()
    g = torch.Generator().manual_seed(B * T + V)
    sep = torch.randint(-1, T + 3, (B, S), generator=g)
    hist = torch.randint(0, S, (B,), generator=g)
    hist[0] = 0
    hist[-1] = S - 1
    sep[0, 0] = -1                                                   # sep + 1 == 0: no text key
    if B > 1:
        sep[1, hist[1]] = T - 1                                      # sep + 1 == T: every key
        sep[-1, S - 1] = T + 2                                       # beyond T
    imask = torch.randint(-2, 4, (B, V), generator=g)
    imask[0, 0] = 7
    sd, hd, md = sep.to(DEV), hist.to(DEV), imask.to(DEV)
    want_t = O.text_key_mask(sep, hist, T).to(torch.uint8)
    want_v = (imask != 0).to(torch.uint8)
    for with_t, with_v in ((True, True), (True, False), (False, True)):
        kt = torch.full((B, T), 0xAB, dtype=torch.uint8, device=DEV)
        kv = torch.full((B, V), 0xAB, dtype=torch.uint8, device=DEV)
        L.check(lib.crct_build_keymasks(sd.data_ptr(), hd.data_ptr(), S, md.data_ptr(), kt.data_ptr() if with_t else None,
                                        kv.data_ptr() if with_v else None, B, T, V, L.current_stream()), "build_keymasks")
        torch.cuda.synchronize()
        assert torch.equal(kt.cpu(), want_t if with_t else torch.full((B, T), 0xAB, dtype=torch.uint8))
        assert torch.equal(kv.cpu(), want_v if with_v else torch.full((B, V), 0xAB, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------- grouped forward / dgrad pairs
@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
def test_grouped_pair_with_epilogues_equals_single_launches(mode, gemm_path):
    """crct_gemm_bf16_grouped with n = 2 and full epilogues (the text / visual pair of a co-attention layer in ONE grid): every
    problem must come out bit-identical to its own single launch -- same K order per output element, whatever the tile.  Grouped
    launches exist for the LDS-DMA kernel only: forced through the register-staged kernel the group runs as single launches."""
    Mt, Mv = 1600, 2880
    if mode == "fwd":       # text FFN-up (bias, GELU, pre-activation kept) || visual FFN-down (bias, dropout, residual add)
        xt, wt, bt = bf(rand(Mt, 768, seed=1)), bf(rand(3072, 768, scale=0.05, seed=2)), rand(3072, seed=3)
        xv, wv, bv = bf(rand(Mv, 1024, seed=4)), bf(rand(1024, 1024, scale=0.05, seed=5)), rand(1024, seed=6)
        res = bf(rand(Mv, 1024, seed=7))
        pre1, pre2 = (torch.empty(Mt, 3072, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        single = [ops.gemm(xt, wt, Mt, 3072, 768, bias=bt, act="gelu", preact_out=pre1),
                  ops.gemm(xv, wv, Mv, 1024, 1024, bias=bv, addend=res, p_drop=0.1, site=7, seed=11)]
        grouped = ops.gemm_grouped([dict(A=xt, B=wt, M=Mt, N=3072, K=768, bias=bt, act="gelu", preact_out=pre2),
                                    dict(A=xv, B=wv, M=Mv, N=1024, K=1024, bias=bv, addend=res, p_drop=0.1, site=7, seed=11)])
        assert torch.equal(pre1, pre2)
    else:                   # text FFN-down dgrad (x gelu'(u)) || visual QKV dgrad (+ residual gradient)
        dyt, wt = bf(rand(Mt, 768, seed=1)), bf(rand(768, 3072, scale=0.05, seed=2))
        u = bf(rand(Mt, 3072, seed=3))
        dyv, wv = bf(rand(Mv, 3072, seed=4)), bf(rand(3072, 1024, scale=0.05, seed=5))
        res = bf(rand(Mv, 1024, seed=6))
        single = [ops.gemm(dyt, wt, Mt, 3072, 768, tb=True, dact_src=u, dact="gelu"),
                  ops.gemm(dyv, wv, Mv, 1024, 3072, tb=True, addend=res)]
        grouped = ops.gemm_grouped([dict(A=dyt, B=wt, M=Mt, N=3072, K=768, tb=True, dact_src=u, dact="gelu"),
                                    dict(A=dyv, B=wv, M=Mv, N=1024, K=3072, tb=True, addend=res)])
    for a, b in zip(single, grouped):
        assert torch.equal(a, b)
        assert float(a.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------- device-scope ordering events
def test_device_events_order_streams_without_the_system_fence(gemm_path):
    """crct/events.py (crct_event_*): record on one stream, wait on another, query / synchronize from the host; the consumer
    stream must see the producer's kernel results (same-device visibility is all these events promise)."""
    # no GEMM here: the test runs under both settings of the GEMM-path switch (gemm_path), which must not reach these kernels
    from crct.events import DeviceEvent, order_streams
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    x = torch.zeros(1 << 22, device=DEV)
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    ev = DeviceEvent()
    for it in range(20):
        with torch.cuda.stream(s1):
            x.add_(1.0)                               # producer
            ev.record(s1)
        ev.wait(s2)
        with torch.cuda.stream(s2):
            y.copy_(x)                                # consumer on another stream
        order_streams(s2, s1)                         # the next producer pass must not overtake the copy
    ev2 = DeviceEvent()
    ev2.record(s2)
    ev2.synchronize()
    assert ev2.query() and ev.query()
    assert float(y.min()) == 20.0 and float(y.max()) == 20.0


def test_attention_fp8_copies_of_context_and_gradients():
    """CrctAttnQuant: the MFMA attention kernels also write ctx as OCP e4m3 and dq / dk / dv as OCP e5m2 (what the attention-output
    and QKV projections' fp8 GEMMs read), quantised from the bf16-rounded results with a device scale, maxima into amax; the bf16
    results are bit-identical to the plain calls, for every wave count; shapes the MFMA kernels do not cover are refused."""
    lib = L.load()
    try:
        for split in (1, 2, 0):
            lib.crct_attention_force_split(split)
            for B, h, Tq, Tk, d in ((3, 16, 100, 100, 64), (3, 32, 40, 100, 32), (5, 12, 20, 20, 64), (5, 16, 36, 36, 64), (4, 32, 20, 36, 32),
                                    (2, 16, 124, 124, 48), (2, 32, 44, 124, 32), (2, 32, 124, 44, 32)):      # the last three: attention_long.hip
                if split and max(Tq, Tk) > 112:
                    continue
                g = torch.Generator().manual_seed(Tq * 1000 + Tk + d)
                q, k, v = (torch.randn(B, T, h * d, generator=g).cuda().bfloat16() for T in (Tq, Tk, Tk))
                do = (torch.randn(B, Tq, h * d, generator=g) * 1e-3).cuda().bfloat16()
                km = torch.ones(B, Tk, dtype=torch.uint8, device="cuda")
                km[:, Tk - 3:] = 0
                ctx = ops.attention_fwd(q, k, v, km, h, d, p_drop=0.1, site=3, seed=9)
                sc, am = torch.tensor([37.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
                ctx2, ctx8 = ops.attention_fwd_q(q, k, v, km, h, d, sc, am, p_drop=0.1, site=3, seed=9)
                assert torch.equal(ctx, ctx2)
                assert torch.equal(ctx8.view(torch.float8_e4m3fn).float(), _q8(ctx, 37.0).float())
                assert float(am.max()) == float(ctx.float().abs().max())
                dq, dk, dv = ops.attention_bwd(q, k, v, km, do, h, d, p_drop=0.1, site=3, seed=9)
                s1, a1 = torch.tensor([3.0e5], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
                s2, a2 = torch.tensor([1.0e5], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
                (dq2, dk2, dv2), (dq8, dk8, dv8) = ops.attention_bwd_q(q, k, v, km, do, h, d, s1, a1, s2, a2, p_drop=0.1, site=3, seed=9)
                assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
                for t, t8, s in ((dq, dq8, 3.0e5), (dk, dk8, 1.0e5), (dv, dv8, 1.0e5)):
                    want = (t.float() * s).clamp(-57344, 57344).to(torch.float8_e5m2)
                    assert torch.equal(t8.view(torch.float8_e5m2).float(), want.float()), (split, Tq, Tk, d)
                if max(Tq, Tk) > 112:      # the long kernels' backward with the forward's row statistics (what the fp8 step runs): same contract
                    lse = torch.empty(B, h, Tq, device=DEV)
                    assert torch.equal(ops.attention_fwd(q, k, v, km, h, d, p_drop=0.1, site=3, seed=9, row_lse=lse), ctx)
                    kept = ops.attention_bwd(q, k, v, km, do, h, d, p_drop=0.1, site=3, seed=9, row_lse=lse, ctx=ctx)
                    a1.zero_(); a2.zero_()
                    kept2, kept8 = ops.attention_bwd_q(q, k, v, km, do, h, d, s1, a1, s2, a2, p_drop=0.1, site=3, seed=9, row_lse=lse, ctx=ctx)
                    for t, t2, t8, s in zip(kept, kept2, kept8, (3.0e5, 1.0e5, 1.0e5)):
                        assert torch.equal(t, t2)
                        assert torch.equal(t8.view(torch.float8_e5m2).float(), (t.float() * s).clamp(-57344, 57344).to(torch.float8_e5m2).float())
                    assert float(a1.max()) == float(kept[0].float().abs().max())
                assert float(a1.max()) == float(dq.float().abs().max())
                assert float(a2.max()) == max(float(dk.float().abs().max()), float(dv.float().abs().max()))
    finally:
        lib.crct_attention_force_split(0)
    assert lib.crct_attention_quant_ok(20, 20, 64) == 1 and lib.crct_attention_quant_ok(20, 20, 40) == 0
    q = torch.randn(2, 8, 4 * 40, device=DEV).bfloat16()
    km = torch.ones(2, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.attention_fwd_q(q, q, q, km, 4, 40, torch.ones(1, device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV))


# ------------------------------------------------------------------------------------------- attention: waves per (batch, head)
def _attn_split_case():
    out = {}
    for name, B, h, Tq, Tk, d in (("self100", 3, 16, 100, 100, 64), ("co40x100", 3, 32, 40, 100, 32), ("self36", 5, 16, 36, 36, 64),
                                  ("self20", 5, 16, 20, 20, 48), ("self64", 2, 16, 64, 50, 48)):
        g = torch.Generator().manual_seed(Tq * 1000 + Tk)
        q = torch.randn(B, Tq, h * d, generator=g).cuda().bfloat16()
        k = torch.randn(B, Tk, h * d, generator=g).cuda().bfloat16()
        v = torch.randn(B, Tk, h * d, generator=g).cuda().bfloat16()
        do = torch.randn(B, Tq, h * d, generator=g).cuda().bfloat16()
        km = torch.ones(B, Tk, dtype=torch.uint8, device="cuda")
        km[:, Tk - 3:] = 0
        out[name + ".ctx"] = ops.attention_fwd(q, k, v, km, h, d, p_drop=0.1, site=3, seed=9).cpu()
        dq, dk, dv = ops.attention_bwd(q, k, v, km, do, h, d, p_drop=0.1, site=3, seed=9)
        out[name + ".dq"], out[name + ".dk"], out[name + ".dv"] = dq.cpu(), dk.cpu(), dv.cpu()
    return out


def test_attention_gives_the_same_bits_for_every_wave_count(gemm_path):
    """attention_mfma.hip splits one (batch, head) over 1, 2 or 4 waves (query tiles, then key tiles); every tile is computed the
    same way in the same summation order, so one wave per pair (crct_attention_force_split(1), the round-1 kernel), two, and the
    default must agree bit for bit -- forward, dq, dk, dv, with dropout, at 7 x 7, 3 x 7, 4 x 4, 3 x 3 and 2 x 2 tiles."""
    # no GEMM here: the test runs under both settings of the GEMM-path switch (gemm_path), which must not reach these kernels
    from crct import lib as L
    lib = L.load()
    res = {}
    try:
        for split in (1, 2, 0):
            lib.crct_attention_force_split(split)
            res[split] = _attn_split_case()
    finally:
        lib.crct_attention_force_split(0)
    assert set(res[1]) == set(res[0]) and len(res[0]) == 20
    for key in res[0]:
        assert torch.equal(res[0][key], res[1][key]), key
        assert torch.equal(res[0][key], res[2][key]), key
        assert float(res[0][key].float().abs().max()) > 0


def test_gemm_refuses_a_leading_dimension_beyond_32_bits():
    """The operands' leading dimensions reach the kernel as preloaded 32-bit scalars (gemm.hip GEMM_HOT_ARGS): a larger one is an error, not
    a truncation."""
    M, N, K = 64, 64, 64
    a = torch.randn(M, K, device="cuda").bfloat16()
    w = torch.randn(N, K, device="cuda").bfloat16()
    g = L.GemmArgs()
    ops._gemm_args(g, a, w, M, N, K)
    g.lda = 1 << 31
    assert L.load().crct_gemm_bf16(C.byref(g), L.current_stream()) != 0
    g.lda, g.ldb = K, 1 << 33
    assert L.load().crct_gemm_bf16(C.byref(g), L.current_stream()) != 0
    g.ldb = K
    assert L.load().crct_gemm_bf16(C.byref(g), L.current_stream()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ GELU / GELU' epilogues (round 5)
def _gelu_points():
    """2^20 pre-activations, bf16-representable: a dense grid over [-9, 9] (beyond +-4 the Abramowitz-Stegun erf is in its tail), a
    logarithmic sweep of small magnitudes of both signs, and N(0, 1.5) draws."""
    g = torch.Generator(device="cpu").manual_seed(5)
    n = 1 << 20
    grid = torch.linspace(-9.0, 9.0, n // 2)
    small = torch.logspace(-6, 0.5, n // 8)
    rnd = torch.randn(n - n // 2 - 2 * (n // 8), generator=g) * 1.5
    u = torch.cat([grid, small, -small, rnd]).bfloat16()
    return u.view(-1, 64).contiguous().to(DEV)


def _bf16_ord(t):
    """bf16 bit patterns mapped to integers that are monotone in the value (distance = number of representable values between)."""
    b = t.view(torch.int16).to(torch.int32) & 0xffff
    return torch.where(b >= 0x8000, 0x8000 - b, b)


def _gelu_epilogue_outputs(gemm_call):
    """(gelu(u), gelu'(u)) as the GEMM epilogues produce them: the forward epilogue on a pre-activation that equals u exactly (u x
    identity), and the data-gradient epilogue  acc * gelu'(dact_src)  on an accumulator that equals 1 exactly."""
    U = _gelu_points()
    M = U.shape[0]
    eye = torch.eye(64, device=DEV).bfloat16()
    y = gemm_call(U, eye, M, 64, 64, act="gelu")
    ones_col = torch.zeros(M, 64, device=DEV).bfloat16()
    ones_col[:, 0] = 1
    wcol = torch.zeros(64, 64, device=DEV).bfloat16()
    wcol[:, 0] = 1
    dy = gemm_call(ones_col, wcol, M, 64, 64, dact_src=U, dact="gelu")
    torch.cuda.synchronize()
    return U, y, dy


def _gelu_check(U, y, dy):
    """(worst distance in bf16 steps, fraction of points that are not the correctly rounded value) for gelu and gelu', against float64
    erf.  Where the exact value is below 1e-5 in magnitude the approximation's ABSOLUTE error bound applies instead (gelu 4.6e-7, gelu'
    3.2e-7: at u = -5 the exact gelu is -1.4e-6, where a bf16 step is 1e-8 -- invisible next to O(1) activations)."""
    u = U.double().cpu()
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    out = []
    for got, ref in ((y, u * cdf), (dy, cdf + u * phi)):
        got = got.cpu()
        ref16 = ref.float().bfloat16()
        big = ref.abs() >= 1e-5
        dist = (_bf16_ord(got) - _bf16_ord(ref16)).abs()[big]
        abs_ok = bool(((got.double() - ref).abs()[~big] <= 1e-6).all())
        out.append((int(dist.max()), float((dist > 0).float().mean()), abs_ok))
    return out


def test_gelu_epilogues_are_within_one_bf16_step_of_libm(gemm_path):
    """the branch-free erf (Abramowitz & Stegun 7.1.26) behind the GELU / GELU' epilogues (vilbert.py:111-117 and its
    derivative) against float64 erf on 2^20 points including |u| > 4: never more than ONE bf16 step from the correctly rounded value,
    and the correctly rounded value itself on >= 99 % of the points (measured: 99.9+ %).  The second bound is what a wrong derivative
    cannot pass: test_a_build_with_a_perturbed_gelu_derivative_is_told_apart."""
    U, y, dy = _gelu_epilogue_outputs(lambda *a, **k: ops.gemm(*a, **k))
    (d0, f0, a0), (d1, f1, a1) = _gelu_check(U, y, dy)
    print("gelu: worst %d bf16 steps, %.4f %% not correctly rounded; gelu': worst %d, %.4f %%" % (d0, 100 * f0, d1, 100 * f1))
    assert d0 <= 1 and d1 <= 1 and a0 and a1, (d0, d1, a0, a1)
    assert f0 <= 0.01 and f1 <= 0.01, (f0, f1)


def _perturbed_library():
    """tools/lab/libcrct_gelu_perturbed.so: this library with gelu' x 1.001 (make -C cqa-crct_amd/csrc perturbed).  A test fixture, not a
    build product (__graft_entry__.build() does not make it): built HERE when it is missing or older than the library under test --
    the same structs must be on both sides of the call -- with the box's own hipcc (a GPU test box has one: without it the test fails)."""
    import os
    import shutil
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(L.LIB_PATH), "..", ".."))
    alt = os.path.join(root, "tools", "lab", "libcrct_gelu_perturbed.so")
    if os.path.exists(alt) and os.path.getmtime(alt) >= os.path.getmtime(L.LIB_PATH):
        return alt
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc) and shutil.which("make"), "no hipcc / make on this box: the perturbed-GELU build cannot be made"
    env = dict(os.environ, HIPCC=hipcc)
    r = subprocess.run(["make", "-C", os.path.join(root, "cqa-crct_amd", "csrc"), "perturbed"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(alt), "make perturbed failed: " + r.stdout[-400:]
    return alt


def test_a_build_with_a_perturbed_gelu_derivative_is_told_apart(gemm_path):
    """The sensitivity of test_gelu_epilogues_are_within_one_bf16_step_of_libm: the same check on a build whose GELU' is off by 1e-3
    relative must FAIL its correct-rounding bound (a quarter of the roundings move), while its unchanged GELU still passes.  The
    second library runs the same GEMM kernel as the library under test (gemm_path): the perturbation is in both of them."""
    alt = _perturbed_library()
    lib2 = C.CDLL(alt)
    lib2.crct_gemm_bf16.restype = C.c_int
    lib2.crct_gemm_bf16.argtypes = [C.POINTER(L.GemmArgs), C.c_void_p]
    lib2.crct_abi_version.restype = C.c_int
    assert lib2.crct_abi_version() == L.load().crct_abi_version()
    lib2.crct_gemm_force_generic(int(gemm_path == "generic"))

    def call2(A, B, M, N, K, **kw):
        g = L.GemmArgs()
        out = ops._gemm_args(g, A, B, M, N, K, **kw)
        assert lib2.crct_gemm_bf16(C.byref(g), L.current_stream()) == 0
        return out
    U2, y2, dy2 = _gelu_epilogue_outputs(call2)
    (_, f0p, _), (d1p, f1p, _) = _gelu_check(U2, y2, dy2)
    print("perturbed build: gelu %.4f %% not correctly rounded (unchanged code), gelu' worst %d steps, %.2f %% not correctly rounded" % (100 * f0p, d1p, 100 * f1p))
    assert f0p <= 0.01                       # its GELU is this build's
    assert f1p > 0.05                        # ... its GELU' is caught: the 1 % bound fails on it


# ------------------------------------------------------------------------------------------- classification head + joint loss
# crct_head_loss (heads.hip: head_rows_kernel + head_reduce_kernel) against an fp64 restatement of oracle.heads_and_losses from the
# poolers' post-ReLU outputs and the fusion.4 post-LeakyReLU rows on, with the host's cls dropout mask.
import heads_ref as HR       # noqa: E402

HEAD_SITE = HR.HEAD_SITE                          # the engine's cls dropout site
HEAD_NSP_COEFF, HEAD_REG_COEFF = HR.HEAD_NSP_COEFF, HR.HEAD_REG_COEFF        # CrctHeadArgs.nsp_coeff / reg_coeff of every launch below
_head_cfg = HR.head_cfg
_HEAD_NORMAL, _HEAD_NONE, _HEAD_BIG, _HEAD_ONE, _HEAD_HALF, _HEAD_ZERO, _HEAD_D5, _HEAD_CLOSE, _HEAD_BOTH0, _HEAD_NONE_R = range(10)


def _head_inputs(B, Hb, seed):
    g = torch.Generator().manual_seed(seed)
    pt = torch.relu(torch.randn(B, Hb, generator=g)).to(torch.bfloat16)
    pv = torch.relu(torch.randn(B, Hb, generator=g)).to(torch.bfloat16)
    w_cls, b_cls = torch.randn(2, Hb, generator=g) * 0.05, torch.tensor([0.1, -0.1])
    fh = torch.nn.functional.leaky_relu(torch.randn(B, 256, generator=g) * 0.7, 0.01)
    w6 = torch.randn(256, generator=g) * 0.08
    w6[0], b6 = 0.5, torch.tensor([0.0625])
    kinds = torch.arange(B) % 10 if B > 1 else torch.zeros(1, dtype=torch.long)
    both0 = kinds == _HEAD_BOTH0
    fh[both0] = 0.0
    fh[both0, 0] = -0.125                       # z = -0.125 * 0.5 + 0.0625 = 0 exactly: r = tanh(0) = 0
    big = (kinds == _HEAD_HALF) | (kinds == _HEAD_D5)
    fh[big] += 2.5 * torch.sign(torch.randn(int(big.sum()), 1, generator=g)) * w6 / w6.norm() ** 2      # |z| ~ 2.5: |r| >= 0.25
    return dict(pt=pt, pv=pv, w_cls=w_cls, b_cls=b_cls, fh=fh.to(torch.bfloat16), w6=w6, b6=b6, kinds=kinds, g=g)


def _d5_boundary_target(rk):
    """An fp32 target t with fl(|fl(rk - t)| / |t|) == 0.05f exactly, or None (about one r in twelve has one)."""
    rk = np.float32(rk)
    for f in (1.05, 0.95):
        t0 = np.float32(rk / f)
        cand = t0 + np.arange(-64, 64, dtype=np.float32) * np.spacing(np.abs(t0))
        with np.errstate(divide="ignore", invalid="ignore"):
            hit = np.nonzero(np.abs(rk - cand) / np.abs(cand) == np.float32(0.05))[0]
        if hit.size:
            return float(cand[hit[0]])
    return None


def _head_tune_boundary_rows(inp, n_cand=192):
    """Rows of the kinds |diff| = 0.5 and d5 = 0.05 need a kernel r with |r| >= 0.25, and one that has a d5 = 0.05 target: one probe launch
    of n_cand variants of each such fus_h row (column 1 moved in steps of 1/64) gives the kernel's r for each; the first that fits is kept.
    r of a row depends on that row alone (one workgroup, fixed summation order)."""
    kinds, fh = inp["kinds"], inp["fh"].float()
    rows = torch.nonzero((kinds == _HEAD_HALF) | (kinds == _HEAD_D5)).flatten().tolist()
    if not rows:
        return
    probe = fh[rows].repeat_interleave(n_cand, 0)
    probe[:, 1] += (torch.arange(n_cand, dtype=torch.float32) / 64.0).repeat(len(rows))
    probe = probe.to(torch.bfloat16)
    n = probe.shape[0]
    pin = dict(inp, pt=torch.zeros(n, 64, dtype=torch.bfloat16), pv=torch.zeros(n, 64, dtype=torch.bfloat16), w_cls=inp["w_cls"][:, :64],
               fh=probe)
    r = _head_launch(pin, torch.zeros(n, 4), None, _head_cfg(use_l1=True, kind_l1=True), grads=False)["reg"][3].view(len(rows), n_cand)
    new = inp["fh"].clone()
    for i, b in enumerate(rows):
        fits = [j for j in range(n_cand) if abs(float(r[i, j])) >= 0.25 and
                (kinds[b] == _HEAD_HALF or _d5_boundary_target(float(r[i, j])) is not None)]
        assert fits, "no variant of row %d fits its boundary" % b
        new[b] = probe[i * n_cand + fits[0]]
    inp["fh"] = new


def _head_targets(inp, r_k, tol):
    """R [B, 4] (gt, needs, tol, scale) per row kind from the kernel's fp32 r (reg[3]) and fp64 r; returns (R, rows whose expectation
    is computed from the kernel's r).  Rows away from a comparison boundary keep a margin of 1e-3 from it."""
    g, kinds = inp["g"], inp["kinds"]
    B = kinds.numel()
    r64 = torch.tanh(inp["fh"].double() @ inp["w6"].double() + inp["b6"].double())
    R = torch.zeros(B, 4, dtype=torch.float32)
    own = torch.zeros(B, dtype=torch.bool)
    rk = r_k.numpy().astype(np.float32)
    for b in range(B):
        kind, r = int(kinds[b]), float(r64[b])
        scale = float(torch.randint(1, 50, (1,), generator=g))
        if kind == _HEAD_HALF and abs(rk[b]) >= 0.25:           # |diff| exactly 0.5: t = r -+ 0.5 is exact for |r| in [0.25, 1)
            R[b] = torch.tensor([float(rk[b] - np.float32(0.5) * np.sign(rk[b])), 1.0, tol, 1.0])
            own[b] = True
            continue
        if kind == _HEAD_D5 and _d5_boundary_target(rk[b]) is not None:     # d5 = |r - t| / |t| exactly 0.05 in fp32
            R[b] = torch.tensor([_d5_boundary_target(rk[b]), 1.0, tol, 1.0])
            own[b] = True
            continue
        if kind == _HEAD_NONE:
            continue                                            # R = [0, 0, 0, 0]
        if kind == _HEAD_NONE_R:
            R[b] = torch.tensor([2.0, 0.0, tol, 5.0])
            continue
        if kind == _HEAD_ONE:
            R[b] = torch.tensor([scale * (1 if b % 4 == 3 else -1), 1.0, tol, scale])    # |target| exactly 1
            continue
        if kind in (_HEAD_ZERO, _HEAD_BOTH0):
            R[b] = torch.tensor([0.0, 1.0, tol, scale])
            continue
        while True:
            if kind == _HEAD_BIG:
                t = float(torch.empty(1).uniform_(1.05, 3.0, generator=g)) * (1 if b % 3 else -1)
            elif kind == _HEAD_CLOSE:
                t = r + float(torch.empty(1).uniform_(-0.6, 0.6, generator=g)) * tol
            else:
                t = r + float(torch.empty(1).uniform_(-1.2, 1.2, generator=g))
            t32 = float(np.float32(np.float32(t * scale) / np.float32(scale)))
            l1 = abs(r - t32)
            if (abs(abs(t32) - 1) > 1e-3 and abs(t32) > 1e-3 and abs(l1 - 0.5) > 1e-3 and abs(l1 - tol) > 1e-3 * max(tol, 1e-3)
                    and abs(l1 / abs(t32) - 0.05) > 1e-3):
                break
        R[b] = torch.tensor([float(np.float32(t * scale)), 1.0, tol, scale])
    return R, own


_head_ref64 = HR.head_ref64      # the fp64 restatement lives in tests/heads_ref.py, shared with tests/test_heads_gpu.py


def _head_launch(inp, R, labels, hc, *, grads=True, g_loss=None, g_nsp=None, g_reg=None, grad_scale=1.0, prefill=0.0, variant=None):
    """One crct_head_loss launch with the settings hc (_head_cfg); outputs start NaN, the parameter gradients pre-filled with
    prefill * randn.  Returns every buffer on the host.
    variant: None, or a dict for crct_head_loss_variant: regressor (L.REGRESSOR_KINDS name), values (the table), snap, and the options
    no_ce_scratch (CE without its scratch), null_reg (fus_h / w_f6 / b_f6 and their gradient pointers NULL), sentinel (a value that
    fills those gradient buffers instead: d_w6 / d_b6 as prefill, d_fh whole).  inp['w6'] / inp['b6'] give fusion.6's shape."""
    B, Hb = inp["pt"].shape
    v = variant or {}
    null_reg = bool(v.get("null_reg"))
    d = lambda t: t.to(DEV).contiguous()         # noqa: E731
    t = dict(pt=d(inp["pt"]), pv=d(inp["pv"]), fh=d(inp["fh"]), w_cls=d(inp["w_cls"]), b_cls=d(inp["b_cls"]), w6=d(inp["w6"]),
             b6=d(inp["b6"]), R=d(R), logits=torch.full((B, 2), float("nan"), device=DEV), reg=torch.full((5, B), float("nan"), device=DEV),
             stats=torch.full((24,), float("nan"), device=DEV), scratch=torch.full((B, 8), float("nan"), device=DEV))
    a = L.HeadArgs()
    a.pooled_t, a.pooled_v = t["pt"].data_ptr(), t["pv"].data_ptr()
    a.w_cls, a.b_cls = t["w_cls"].data_ptr(), t["b_cls"].data_ptr()
    if not null_reg:
        a.fus_h, a.w_f6, a.b_f6 = t["fh"].data_ptr(), t["w6"].data_ptr(), t["b6"].data_ptr()
    a.R = t["R"].data_ptr()
    if labels is not None:
        t["labels"] = d(labels)
        a.labels = t["labels"].data_ptr()
    a.logits, a.reg, a.stats, a.scratch = t["logits"].data_ptr(), t["reg"].data_ptr(), t["stats"].data_ptr(), t["scratch"].data_ptr()
    if grads:
        g = torch.Generator().manual_seed(B + Hb)
        t.update(d_pt=torch.full((B, Hb), float("nan"), device=DEV, dtype=torch.bfloat16), d_pv=torch.full((B, Hb), float("nan"), device=DEV, dtype=torch.bfloat16),
                 d_fh=torch.full((B, 256), float("nan"), device=DEV, dtype=torch.bfloat16),
                 d_w_cls=d(torch.randn(2, Hb, generator=g) * prefill), d_b_cls=d(torch.randn(2, generator=g) * prefill),
                 d_w6=d(torch.randn(*inp["w6"].shape, generator=g) * prefill), d_b6=d(torch.randn(*inp["b6"].shape, generator=g) * prefill))
        if "sentinel" in v:
            for k in ("d_fh", "d_w6", "d_b6"):
                t[k].fill_(v["sentinel"])
        t["prefill"] = {k: t[k].cpu() for k in ("d_w_cls", "d_b_cls", "d_w6", "d_b6")}
        a.d_pooled_t, a.d_pooled_v = t["d_pt"].data_ptr(), t["d_pv"].data_ptr()
        a.d_w_cls, a.d_b_cls = t["d_w_cls"].data_ptr(), t["d_b_cls"].data_ptr()
        if not null_reg:
            a.d_fus_h, a.d_w_f6, a.d_b_f6 = t["d_fh"].data_ptr(), t["d_w6"].data_ptr(), t["d_b6"].data_ptr()
    for k, x in (("g_loss_dev", g_loss), ("g_nsp_dev", g_nsp), ("g_reg_dev", g_reg)):
        if x is not None:
            t[k] = d(x.float().reshape(-1))
            setattr(a, k, t[k].data_ptr())
    a.B, a.Hb, a.fusion_sum, a.use_l1, a.kind_l1 = B, Hb, int(hc["fusion_sum"]), int(hc["use_l1"]), int(hc["kind_l1"])
    a.tol_margin, a.nsp_coeff, a.reg_coeff, a.grad_scale = hc["tol"], HEAD_NSP_COEFF, HEAD_REG_COEFF, grad_scale
    a.drop_thr, a.drop_scale, a.drop_site = ops._drop(hc["p"], HEAD_SITE)
    a.seed = hc["seed"]
    if variant is None:
        L.check(L.load().crct_head_loss(C.byref(a), L.current_stream()), "head_loss")
    else:
        va = L.HeadVariantArgs()
        va.h = a
        va.variant.dataset, va.variant.regressor = L.DATASET_KINDS["dvqa"], L.REGRESSOR_KINDS[v["regressor"]]
        values = v.get("values", ())
        va.variant.n_values = v.get("n_values", len(values))
        for i, x in enumerate(values):
            va.variant.values[i] = x
        va.snap = int(v.get("snap", 0))
        if v["regressor"] == "ce" and not v.get("no_ce_scratch"):
            t["ce"] = torch.full((B, L.CE_CLASSES), float("nan"), device=DEV)
            va.ce_scratch = t["ce"].data_ptr()
        L.check(L.load().crct_head_loss_variant(C.byref(va), L.current_stream()), "head_loss_variant")
    torch.cuda.synchronize()
    return {k: (x.cpu() if torch.is_tensor(x) else x) for k, x in t.items()}


def _assert_bf16_grad(got, ref, scale, what):
    """bf16 gradient seeds: within one bf16 step of fp64, plus 2^-16 of `scale`, the magnitude |dl0 w0| + |dl1 w1| (times the scale and the
    other pooler) of the two terms the kernel adds.  The slack is the error of the kernel's logit gradients dl = (expf(l - lse) - y) w:
    its logits are fp32 sums over Hb products, and where the two columns of w_cls are alike the two terms cancel and leave that error
    exposed.  Measured worst over every case of test_head_loss_against_fp64: 3.6e-6 of `scale` (2^-18); the bound sits 4 x above."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    tol = _bf16_step(torch.maximum(got.abs(), ref.abs())) + 2.0 ** -16 * scale
    bad = err > tol
    assert not bool(bad.any()), "%s: %d elements beyond one bf16 step, first at %s (got %r, fp64 %r)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]))


@pytest.mark.parametrize("Hb", [64, 1024])
@pytest.mark.parametrize("B", [1, 7, 80, 300])
def test_head_loss_against_fp64(B, Hb):
    """Every output of crct_head_loss: logits, the five reg rows, stats[0..16] (counts exact), the bf16 gradient seeds and the fp32 parameter
    gradients (added to pre-filled buffers), for both fusions, p = 0 and 0.1, L1 and SmoothL1 (kind_l1 = 1 / 0), the three device
    upstream-gradient pointers with grad_scale != 1, labels -1 (a batch of them only, too) and the evaluation form.  Rows cover
    R = [0, 0, 0, 0], |target| > 1 and exactly 1, |diff| exactly 0.5, target 0, both zero, d5 exactly 0.05 and |diff| under tol_margin."""
    tol = 0.01
    inp = _head_inputs(B, Hb, seed=B * 7 + Hb)
    _head_tune_boundary_rows(inp)
    g = inp["g"]
    labels = torch.randint(0, 2, (B,), generator=g)
    labels[torch.arange(B) % 5 == 2] = -1
    combos = [(0, 0.0, False, False, "default"), (1, 0.1, True, True, "loss_dev"), (0, 0.1, False, False, "nsp_reg_dev"),
              (1, 0.0, True, False, "loss_dev")]
    r_k = None
    for i, (fusion_sum, p, use_l1, kind_l1, upstream) in enumerate(combos):
        seed = DROP_SEEDS[i % 2] + B
        if r_k is None:      # reg[3] = tanh(z) depends on neither R nor the labels: one launch gives the kernel's r for the boundary rows
            r_k = _head_launch(inp, torch.zeros(B, 4), labels, _head_cfg(seed=seed, use_l1=True, kind_l1=True, tol=tol), grads=False)["reg"][3]
            R, own = _head_targets(inp, r_k, tol)
            kinds = inp["kinds"]
            assert torch.equal(own, (kinds == _HEAD_HALF) | (kinds == _HEAD_D5)), "boundary rows fell back to ordinary ones"
        lab = labels if i != 3 else torch.full((B,), -1, dtype=torch.long)      # every label ignored
        gs = (1.0, 2.5, 0.5, 1.0)[i]
        g_loss = torch.tensor([0.37]) if upstream == "loss_dev" else None
        g_nsp = torch.tensor([1.3]) if upstream == "nsp_reg_dev" else None
        g_reg = torch.linspace(-0.5, 1.5, B) if upstream == "nsp_reg_dev" else None
        if upstream == "nsp_reg_dev":
            gn, gr = 1.3 * gs, g_reg.double() * gs
        else:
            gl = (0.37 if g_loss is not None else 1.0) * gs
            gn, gr = HEAD_NSP_COEFF * gl, torch.full((B,), HEAD_REG_COEFF * gl / B, dtype=torch.float64)
        keep = torch.from_numpy(DR.keep_rowmajor(seed, HEAD_SITE, B, Hb, p)) if p else torch.ones(B, Hb, dtype=torch.bool)
        hc = _head_cfg(p=p, seed=seed, fusion_sum=fusion_sum, use_l1=use_l1, kind_l1=kind_l1, tol=tol)
        out = _head_launch(inp, R, lab, hc, g_loss=g_loss, g_nsp=g_nsp, g_reg=g_reg, grad_scale=gs, prefill=0.3)
        ref, grads, reg_mag = _head_ref64(inp, R, lab, keep, hc, g_nsp=gn, g_reg=gr, r_k=r_k, own=own)
        what = "B=%d Hb=%d combo %d" % (B, Hb, i)
        assert torch.equal(out["reg"][3], r_k), what + ": r changed between launches"
        _assert_sums(out["logits"], ref["logits"], ref["logit_mag"], what + ": logits")
        for k in range(5):
            _assert_sums(out["reg"][k], ref["reg"][k], reg_mag[k], what + ": reg[%d]" % k)
        st = out["stats"][:17].double()
        counts = [3, 4, 5, 6, 7, 9, 13, 14, 15, 16]
        assert torch.equal(st[counts], ref["stats"][counts]), (what, st[counts].tolist(), ref["stats"][counts].tolist())
        fl = [0, 1, 2, 8, 10, 11, 12]
        _assert_sums(st[fl], ref["stats"][fl], ref["stats"][fl].abs() + 1e-2, what + ": stats")
        if i == 3:
            # every label -1: the kernel's NSP loss is 0 (stats[1], stats[10]) and no NSP gradient flows; torch's cross_entropy with
            # ignore_index = -1 returns NaN there
            assert float(st[1]) == 0.0 and float(st[10]) == 0.0 and int(st[6]) == 0
            assert bool(torch.isnan(torch.nn.functional.cross_entropy(ref["logits"], lab, ignore_index=-1)))
        assert B < 10 or 0 < int(st[4]) < int(st[3]) and 0 < int(st[5]) < int(st[3])
        fd = (inp["pt"].double() + inp["pv"].double() if fusion_sum else inp["pt"].double() * inp["pv"].double()) * keep / (1 - p)
        dl = out["scratch"][:, :2].double()
        wa = inp["w_cls"].double().abs()
        df_mag = (dl[:, :1].abs() * wa[0] + dl[:, 1:].abs() * wa[1]) / (1 - p)          # |dl0 w0| + |dl1 w1|, times the scale
        _assert_bf16_grad(out["d_pt"], grads["d_pt"], df_mag * (1 if fusion_sum else inp["pv"].double()), what + ": d_pooled_t")
        _assert_bf16_grad(out["d_pv"], grads["d_pv"], df_mag * (1 if fusion_sum else inp["pt"].double()), what + ": d_pooled_v")
        _assert_bf16_grad(out["d_fh"], grads["d_fh"], grads["d_fh"].abs(), what + ": d_fus_h")
        dz = out["scratch"][:, 2].double().abs()
        mags = dict(d_w_cls=dl.abs().t() @ fd.abs(), d_b_cls=dl.abs().sum(0), d_w6=dz @ inp["fh"].double().abs(), d_b6=dz.sum().reshape(1))
        for k in ("d_w_cls", "d_b_cls", "d_w6", "d_b6"):
            pre = out["prefill"][k].double()
            _assert_sums(out[k], pre + grads[k], mags[k] + pre.abs(), what + ": " + k)
    # evaluation: no labels, kind_l1 = 1, no gradient outputs
    hc = _head_cfg(use_l1=False, kind_l1=True, tol=tol)
    out = _head_launch(inp, R, None, hc, grads=False)
    ref, _, reg_mag = _head_ref64(inp, R, None, torch.ones(B, Hb, dtype=torch.bool), hc, g_nsp=1.0, g_reg=torch.zeros(B, dtype=torch.float64),
                                  r_k=r_k, own=own)
    _assert_sums(out["logits"], ref["logits"], ref["logit_mag"], "eval: logits")
    for k in range(5):
        _assert_sums(out["reg"][k], ref["reg"][k], reg_mag[k], "eval: reg[%d]" % k)
    st = out["stats"][:17].double()
    assert torch.equal(st[[0, 1, 6, 8, 10]], torch.zeros(5, dtype=torch.float64))
    assert torch.equal(st[[3, 4, 5, 7, 9, 13, 14, 15, 16]], ref["stats"][[3, 4, 5, 7, 9, 13, 14, 15, 16]])
    fl = [2, 11, 12]                              # the reg mean and the L1 / d5 averages over the rows that need regression
    _assert_sums(st[fl], ref["stats"][fl], ref["stats"][fl].abs() + 1e-2, "eval: stats")


def test_head_dropout_mask_is_the_host_stream():
    """head_keep's numbering (b Hb + c, groups across rows: B odd, Hb = 64 / 1032) through the zeros of d_pooled_t: strictly positive
    pooler outputs and a valid label on every row leave no other zero; head_rows_kernel's logits and head_reduce_kernel's d_w_cls
    regenerate the same mask (fp64 with it)."""
    for B, Hb in ((7, 64), (13, 1032), (300, 64)):
        inp = _head_inputs(B, Hb, seed=B + Hb)
        inp["pt"] = (inp["pt"].float().abs() + 0.05).to(torch.bfloat16)
        inp["pv"] = (inp["pv"].float().abs() + 0.05).to(torch.bfloat16)
        labels = torch.arange(B) % 2
        R = torch.zeros(B, 4)
        for seed in DROP_SEEDS:
            keep = torch.from_numpy(DR.keep_rowmajor(seed, HEAD_SITE, B, Hb, 0.1))
            hc = _head_cfg(p=0.1, seed=seed)
            out = _head_launch(inp, R, labels, hc)
            assert bool((out["d_pv"] != 0).any())
            assert torch.equal(out["d_pt"] != 0, keep), (B, Hb, int(((out["d_pt"] != 0) != keep).sum()))
            assert torch.equal(out["d_pv"] != 0, keep)
            ref, grads, _ = _head_ref64(inp, R, labels, keep, hc, g_nsp=HEAD_NSP_COEFF, g_reg=torch.full((B,), HEAD_REG_COEFF / B, dtype=torch.float64),
                                        r_k=out["reg"][3], own=torch.zeros(B, dtype=torch.bool))
            _assert_sums(out["logits"], ref["logits"], ref["logit_mag"], "logits")
            fd = inp["pt"].double() * inp["pv"].double() * keep / 0.9
            dl = out["scratch"][:, :2].double()
            pre = out["prefill"]["d_w_cls"].double()
            _assert_sums(out["d_w_cls"], pre + grads["d_w_cls"], dl.abs().t() @ fd.abs() + pre.abs(), "d_w_cls")


# ------------------------------------------------------------------------------------------- GEMM bit for bit against fp64
# tests/gemm_ref.py: integer-valued operands scaled by powers of two, every entry non-zero, every partial sum below 2^24 (2^20 for
# fp8) in units of the product's scale.  The fp32 accumulator of any tile, K order or split is then the fp64 product, so an fp32
# output must equal the fp64 reference bit for bit and a bf16 output its round-to-nearest-even (ties included).  A dropped, doubled or
# misplaced product, a ragged-tail store into a neighbour or an accumulator rounded on the way fails here however small it is next
# to the largest output.  Every case also checks, through the launch log, which configuration (and split) actually ran, and every
# output lives inside a larger buffer whose elements outside [M, N] must keep the sentinel.
import gemm_ref as GR        # noqa: E402

SENT = -1.5 * 2.0 ** 100      # exact in bf16 and fp32; no exact result comes near it
GEMM_CFGS = (0, 3, 4, 9, 11, 12, 15, 50)


def _logged(fn):
    """fn() under crct_launch_log_enable: (its result, [(cfg, split_k, n_problems)] of every GEMM launch it made)."""
    lib = L.load()
    lib.crct_launch_log_enable(1)
    try:
        out = fn()
    finally:
        recs = []
        for i in range(lib.crct_launch_log_count()):
            r = L.LaunchRec()
            lib.crct_launch_log_read(i, C.byref(r))
            recs.append((r.cfg, r.split_k, r.n_problems))
        lib.crct_launch_log_enable(0)
    return out, recs


def _ran_cfg(gemm_path, tile, M, N, K, ta=False):
    """The configuration crct_gemm_launch runs for an explicit `tile`: the id itself on the LDS-DMA kernel, else 16 + the register-staged
    kernel's tile (an id 0 - 3 is taken as that tile, 0 meaning 1; any other id, or -1, as crct_gemm_pick_tile's)."""
    if gemm_path == "pipelined" and K % 64 == 0 and tile >= 0:
        return tile
    t = tile if 0 <= tile <= 3 else L.load().crct_gemm_pick_tile(M, N)
    return 16 + (1 if t == 0 else t)


def _canvas(M, N, ld, dtype, extra_rows=3, inner=None):
    """[M + extra_rows][ld] buffer of the sentinel, [M][N] = inner (or the sentinel)."""
    buf = torch.full((M + extra_rows, ld), SENT, device=DEV, dtype=dtype)
    if inner is not None:
        buf[:M, :N] = inner.to(dtype)
    return buf


def _assert_canary(buf, M, N, what):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:M, :N] = False
    out = buf[mask].double()
    bad = out != SENT
    assert not bool(bad.any()), "%s: %d elements outside [%d, %d] of the output buffer were written" % (what, int(bad.sum()), M, N)


def _assert_bits(got, ref, what):
    g, r = got.double(), ref.double().to(got.device)
    bad = g != r
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ from the exact result, first at %s (got %r, exact %r)"
                             % (what, int(bad.sum()), bad.numel(), i, float(g[i]), float(r[i])))


def _operands(layout, M, N, K, amax, bmax, seed, ea=-3, eb=-5, extra=0):
    """(A, B, layout keywords, exact product [M][N] fp64): A, B bf16 on the GPU with leading dimensions larger than their rows."""
    a, b = GR.operands(M, N, K, amax, bmax, seed, ea=ea, eb=eb, extra=extra)
    a, b = a.to(DEV), b.to(DEV)
    ref = GR.ref_nt(a, b)
    if layout == "nt":
        A, B, kw = GR.strided(a, K + 16), GR.strided(b, K + 8), dict(lda=K + 16, ldb=K + 8)
    elif layout == "tb":
        A, B, kw = GR.strided(a, K + 16), GR.strided(b.t(), N + 8), dict(tb=True, lda=K + 16, ldb=N + 8)
    else:
        A, B, kw = GR.strided(a.t(), M + 8), GR.strided(b.t(), N + 8), dict(ta=True, tb=True, lda=M + 8, ldb=N + 8)
    return bf(A), bf(B), kw, ref


def _run_exact(A, B, M, N, K, kw, ref, expect, what, out_f32):
    """One launch into a sentinel canvas (ldc = N + 24), checked bit for bit against the exact product and through the launch log."""
    buf = _canvas(M, N, N + 24, torch.float32 if out_f32 else torch.bfloat16)
    _, recs = _logged(lambda: ops.gemm(A, B, M, N, K, out=buf, ldc=N + 24, **kw))
    assert recs == [expect], (what, recs, expect)
    _assert_bits(buf[:M, :N], GR.f32(ref) if out_f32 else GR.bf16(ref), what)
    _assert_canary(buf, M, N, what)
    return buf[:M, :N]


@pytest.mark.parametrize("layout", ["nt", "tb", "tt"])
@pytest.mark.parametrize("tile", GEMM_CFGS)
def test_gemm_every_configuration_and_layout_bit_for_bit(tile, layout, gemm_path):
    """Every built bf16 configuration in every layout: forward (NT), data gradient (tb) and weight gradient (ta + tb), M = 128 k +- 1
    (or 128 k + 8 where M % 8 == 0 is required) and N = 8 (mod 64): ragged in both tile dimensions.  K = 64 (one K step, shorter than
    every ring), 128 and 192 (2 - 3 steps against the 3- and 4-stage prologues) and 3072."""
    M = 264 if layout == "tt" else (255 if tile in (3, 11, 15) else 257)
    N = 200
    ties = 0
    for K in (64, 128, 192, 3072):
        A, B, kw, ref = _operands(layout, M, N, K, 48, 48, seed=K + tile)
        expect = (_ran_cfg(gemm_path, tile, M, N, K), 1, 1)
        what = "cfg %d %s K=%d" % (tile, layout, K)
        _run_exact(A, B, M, N, K, dict(kw, tile=tile), ref, expect, what + " fp32", True)
        _run_exact(A, B, M, N, K, dict(kw, tile=tile), ref, expect, what + " bf16", False)
        ties += GR.bf16_ties(ref)
    assert ties > 0                                  # round-to-nearest-even was exercised on exact ties


# register-staged kernel: K % 64 != 0 or N % 8 == 4 (no LDS-DMA path), and weight gradients of any R; its three tiles
# (crct_gemm_pick_tile: 1 = 4x2 waves of 128 x 64, 2 = 2x4 of 64 x 128, 3 = 2x2 of 64 x 64) reached by the output shape
_RS_CASES = [("nt", 100, 4, 8, 3), ("nt", 77, 12, 72, 3), ("nt", 130, 100, 776, 3), ("tb", 97, 104, 776, 3), ("tb", 33, 8, 8, 3),
             ("nt", 1700, 1092, 72, 1), ("nt", 7681, 136, 8, 2), ("tb", 7681, 136, 72, 2), ("tb", 1700, 1096, 776, 1)]
_RS_WGRAD_R = (1, 7, 63, 65, 129, 257, 1601)


@pytest.mark.parametrize("layout,M,N,K,t", _RS_CASES)
def test_gemm_register_staged_kernel_bit_for_bit(layout, M, N, K, t, gemm_path):
    assert L.load().crct_gemm_pick_tile(M, N) == t or (t == 1 and L.load().crct_gemm_pick_tile(M, N) == 0)
    A, B, kw, ref = _operands(layout, M, N, K, 64, 64, seed=M + N + K)
    for out_f32 in (True, False):
        _run_exact(A, B, M, N, K, kw, ref, (16 + t, 1, 1), "%s %dx%dx%d" % (layout, M, N, K), out_f32)


@pytest.mark.parametrize("M,N,t", [(136, 200, 3), (1704, 1096, 1), (7688, 136, 2)])
def test_gemm_register_staged_weight_gradients_of_any_R(M, N, t, gemm_path):
    """ta + tb with R (the contraction) not a multiple of 64 -- or of 8 -- always runs the register-staged kernel; accumulate onto a
    prefilled fp32 gradient as the step does."""
    assert L.load().crct_gemm_pick_tile(M, N) in ((0, 1) if t == 1 else (t,))
    for R in (_RS_WGRAD_R if M < 1000 else (1, 65, 1601)):
        A, B, kw, ref = _operands("tt", M, N, R, 64, 64, seed=R, extra=1 << 12)
        pre = GR.unit_ints((M, N), 64, R + 5, 2.0 ** -8).to(DEV)
        buf = _canvas(M, N, N + 8, torch.float32, inner=pre)
        _, recs = _logged(lambda: ops.gemm(A, B, M, N, R, out=buf, ldc=N + 8, accumulate=True, **kw))
        assert recs == [(16 + t, 1, 1)], (R, recs)
        _assert_bits(buf[:M, :N], GR.f32(ref + pre), "wgrad %dx%d R=%d" % (M, N, R))
        _assert_canary(buf, M, N, "wgrad R=%d" % R)


def _epi_case(layout, M, N, K, seed):
    """Operands at a magnitude where GELU / tanh are not trivial (|acc| up to 12, typically ~0.3), unit 2^-12."""
    return _operands(layout, M, N, K, 16, 16, seed, ea=-6, eb=-6, extra=1 << 16)


@pytest.mark.parametrize("layout,M,N,K,tile", [("nt", 333, 264, 192, 15), ("tb", 257, 136, 128, 50), ("nt", 130, 100, 72, -1),
                                                ("tb", 255, 200, 3072, 9)])
def test_gemm_exact_epilogues_bit_for_bit(layout, M, N, K, tile, gemm_path):
    """bias, preact_out, relu, dropout at p = 0.5 / 0.75 (scale 2 / 4: exact) and 0.1 (one fp32 multiply by the kernel's scale), bf16
    and fp32 addend, accumulate onto bf16 and fp32 outputs, c_cached: all bit for bit.  preact_out lives in a sentinel canvas too
    (ld_aux > N)."""
    unit = 2.0 ** -12
    A, B, kw, acc = _epi_case(layout, M, N, K, seed=M + K)
    cfg = _ran_cfg(gemm_path, tile, M, N, K) if tile >= 0 else 16 + L.load().crct_gemm_pick_tile(M, N)
    kw = dict(kw, tile=tile)
    bias = GR.unit_ints((N,), 255, 1, unit * 4).to(DEV)
    add_b = GR.unit_ints((M, N), 255, 2, unit * 8).to(DEV)               # bf16-exact: <= 8 significant bits
    add_f = GR.unit_ints((M, N), 255, 3, unit).to(DEV) * 33               # fp32 only
    pre_b = GR.unit_ints((M, N), 255, 4, unit * 16).to(DEV)
    pre_f = GR.unit_ints((M, N), 255, 5, unit).to(DEV) * 77
    ties = 0
    for seed, site, p in ((DROP_SEEDS[0], 16, 0.5), (DROP_SEEDS[1], 41, 0.75), (DROP_SEEDS[0], 3, 0.1)):
        keep = host_keep(seed, site, M, N, p)
        ds = 1.0 / (1.0 - p)
        drop = dict(p_drop=p, site=site, seed=seed)
        # bias -> preact_out -> relu -> dropout -> bf16 addend -> bf16 store
        pre = _canvas(M, N, N + 16, torch.bfloat16)
        y = _canvas(M, N, N + 24, torch.bfloat16)
        _, recs = _logged(lambda: ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, bias=bias.float(), act="relu", preact_out=pre, ld_aux=N + 16,
                                           addend=bf(add_b), **drop, **kw))
        assert recs == [(cfg, 1, 1)], recs
        r = GR.epilogue(acc, bias=bias, act="relu", keep=keep, drop_scale=ds, addend=add_b, out="bf16")
        what = "%s p=%g" % (layout, p)
        _assert_bits(pre[:M, :N], r["pre"], what + ": preact_out")
        _assert_bits(y[:M, :N], r["y"], what + ": bias relu dropout bf16-addend")
        _assert_canary(pre, M, N, what + ": preact_out")
        _assert_canary(y, M, N, what + ": y")
        ties += GR.bf16_ties(r["v"])
        # bias -> dropout -> fp32 addend -> fp32 c_cached store (the fp32 residual stream)
        y = _canvas(M, N, N + 8, torch.float32)
        ops.gemm(A, B, M, N, K, out=y, ldc=N + 8, bias=bias.float(), addend=add_f.float(), c_cached=True, **drop, **kw)
        _assert_bits(y[:M, :N], GR.epilogue(acc, bias=bias, keep=keep, drop_scale=ds, addend=add_f, out="f32")["y"], what + ": c_cached")
        _assert_canary(y, M, N, what + ": c_cached")
        if p == 0.1:
            continue                # below: products and sums of two roundings (a fused multiply-add may take one)
        # dropout -> bf16 addend -> accumulate onto bf16 / onto fp32
        y = _canvas(M, N, N + 24, torch.bfloat16, inner=pre_b)
        ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, addend=bf(add_b), accumulate=True, **drop, **kw)
        r = GR.epilogue(acc, keep=keep, drop_scale=ds, addend=add_b, prev=pre_b, out="bf16")
        _assert_bits(y[:M, :N], r["y"], what + ": accumulate onto bf16")
        _assert_canary(y, M, N, what + ": accumulate bf16")
        ties += GR.bf16_ties(r["v"] + pre_b)
        y = _canvas(M, N, N + 8, torch.float32, inner=pre_f)
        ops.gemm(A, B, M, N, K, out=y, ldc=N + 8, bias=bias.float(), addend=bf(add_b), accumulate=True, **drop, **kw)
        r = GR.epilogue(acc, bias=bias, keep=keep, drop_scale=ds, addend=add_b, prev=pre_f, out="f32")
        _assert_bits(y[:M, :N], r["y"], what + ": accumulate onto fp32")
        _assert_canary(y, M, N, what + ": accumulate fp32")
    assert ties > 0


@pytest.mark.parametrize("layout,M,N,K,tile", [("nt", 333, 264, 192, 15), ("nt", 130, 100, 72, -1), ("tb", 257, 200, 768, 4)])
def test_gemm_rounded_epilogues_within_one_rounding(layout, M, N, K, tile, gemm_path):
    """gelu, tanh, leaky, dact gelu / leaky and dropout at p = 0.1 in front of an addend: fp64 of the exact accumulator, the bf16 output
    within one bf16 step (+ 2^-20 of the terms' magnitude: the kernel's own fp32 roundings)."""
    unit = 2.0 ** -12
    A, B, kw, acc = _epi_case(layout, M, N, K, seed=M + N)
    kw = dict(kw, tile=tile)
    bias = GR.unit_ints((N,), 255, 11, unit * 4).to(DEV)
    add_b = GR.unit_ints((M, N), 255, 12, unit * 8).to(DEV)
    src = bf(rand(M, N, scale=1.5, seed=13)).double()
    for act in ("gelu", "tanh", "leaky"):
        y = _canvas(M, N, N + 24, torch.bfloat16)
        ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, bias=bias.float(), act=act, **kw)
        r = GR.epilogue(acc, bias=bias, act=act)
        _assert_within_bf16_step(y[:M, :N], r["v"], r["v"].abs().cpu(), "%s %s" % (layout, act))
        _assert_canary(y, M, N, act)
    for dact, s in (("gelu", src), ("leaky", src)):
        y = _canvas(M, N, N + 24, torch.bfloat16)
        ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, dact_src=bf(s), dact=dact, **kw)
        r = GR.epilogue(acc, dact=dact, dact_src=s)
        # gelu'(s) = 0.5 (1 + erf(s / sqrt 2)) + s phi(s): its two terms cancel near s = -0.75, where the fp32 evaluation keeps an error
        # of their magnitude, not of the result's
        terms = 0.5 * (1 + torch.erf(s / math.sqrt(2)).abs()) + (s * torch.exp(-0.5 * s * s)).abs() / math.sqrt(2 * math.pi)
        _assert_within_bf16_step(y[:M, :N], r["v"], (acc.abs() * terms).cpu(), "%s dact %s" % (layout, dact))
        _assert_canary(y, M, N, "dact " + dact)
    keep = host_keep(DROP_SEEDS[1], 23, M, N, 0.1)
    y = _canvas(M, N, N + 24, torch.bfloat16)
    ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, bias=bias.float(), act="gelu", p_drop=0.1, site=23, seed=DROP_SEEDS[1], addend=bf(add_b), **kw)
    r = GR.epilogue(acc, bias=bias, act="gelu", keep=keep, drop_scale=1.0 / 0.9, addend=add_b)
    _assert_within_bf16_step(y[:M, :N], r["v"], (r["v"] - add_b).abs().cpu() + add_b.abs().cpu(), layout + " gelu dropout 0.1 addend")


@pytest.mark.parametrize("tile", (4, 9, 12, 15))
def test_gemm_split_k_bit_for_bit(tile, gemm_path):
    """Split-K S = 2 .. 8 with the full epilogue: K / 64 = 2 S (the smallest split allowed), 2 S + 1 and 48 (slices of uneven length) run
    split, 2 S - 1 falls back to one unsplit launch -- both checked through the launch log -- and every result is the exact one (so also
    the unsplit bits).  On the register-staged kernel (gemm_path) the request runs unsplit."""
    M, N = 257, 200
    unit = 2.0 ** -8
    bias = GR.unit_ints((N,), 255, 21, unit).to(DEV)
    add_b = GR.unit_ints((M, N), 255, 22, unit * 4).to(DEV)
    cases = [(S, nk) for S in range(2, 9) for nk in (2 * S - 1, 2 * S, 2 * S + 1)] + [(3, 48), (5, 48), (8, 48)]
    for S, nk in cases:
        K = 64 * nk
        layout = "tb" if S % 2 else "nt"
        A, B, kw, acc = _operands(layout, M, N, K, 48, 48, seed=S * 100 + nk, extra=1 << 12)
        keep = host_keep(DROP_SEEDS[0], 17, M, N, 0.5)
        split = S if (gemm_path == "pipelined" and nk >= 2 * S) else 1
        expect = (_ran_cfg(gemm_path, tile, M, N, K), split, 1)
        pre = _canvas(M, N, N + 8, torch.bfloat16)
        y = _canvas(M, N, N + 24, torch.bfloat16)
        _, recs = _logged(lambda: ops.gemm(A, B, M, N, K, out=y, ldc=N + 24, bias=bias.float(), preact_out=pre, ld_aux=N + 8, act="relu",
                                           p_drop=0.5, site=17, seed=DROP_SEEDS[0], addend=bf(add_b), tile=tile, split_k=S, **kw))
        assert recs == [expect], (S, nk, recs, expect)
        r = GR.epilogue(acc, bias=bias, act="relu", keep=keep, drop_scale=2.0, addend=add_b)
        what = "cfg %d S=%d K/64=%d" % (tile, S, nk)
        _assert_bits(y[:M, :N], r["y"], what)
        _assert_bits(pre[:M, :N], r["pre"], what + ": preact_out")
        _assert_canary(y, M, N, what)
        _assert_canary(pre, M, N, what + ": preact_out")
        y32 = _canvas(M, N, N + 8, torch.float32)
        ops.gemm(A, B, M, N, K, out=y32, ldc=N + 8, tile=tile, split_k=S, **kw)
        _assert_bits(y32[:M, :N], GR.f32(acc), what + ": fp32")
        _assert_canary(y32, M, N, what + ": fp32")


def _wgrad_rowsum_case(M, N, R, seed):
    A, B, kw, ref = _operands("tt", M, N, R, 32, 32, seed=seed, extra=1 << 14)
    pre = GR.unit_ints((M, N), 64, seed + 1, 2.0 ** -8).to(DEV)
    rs_pre = GR.unit_ints((M,), 64, seed + 2, 2.0 ** -3).to(DEV)
    # rowsum_out[m] += sum_k A'[m][k]: the column sums of dy as stored, [R][M] -> exact (integers * 2^-3, |sum| < 2^24 units)
    rs_ref = rs_pre + A[:R, :M].double().sum(0)
    return A, B, kw, ref, pre, rs_pre, rs_ref


def test_gemm_rowsum_bias_gradient_bit_for_bit(gemm_path):
    """rowsum_out (the bias gradient of a weight-gradient launch), single on every configuration that runs weight gradients and grouped,
    exact, in a sentinel canvas of M + 8 words.  LDS-DMA kernel only: on the register-staged kernel (gemm_path) a request is refused."""
    if gemm_path == "generic":
        A, B, kw, *_ = _wgrad_rowsum_case(136, 200, 192, 1)
        with pytest.raises(RuntimeError, match="gemm"):
            ops.gemm(A, B, 136, 200, 192, out=torch.zeros(136, 200, device=DEV), accumulate=True, rowsum_out=torch.zeros(136, device=DEV), **kw)
        return
    for tile in GEMM_CFGS:
        for M, N, R in ((136, 200, 192), (264, 72, 3072)):
            A, B, kw, ref, pre, rs_pre, rs_ref = _wgrad_rowsum_case(M, N, R, seed=tile * 7 + R)
            out = _canvas(M, N, N + 8, torch.float32, inner=pre)
            rs = torch.full((M + 8,), SENT, device=DEV)
            rs[:M] = rs_pre.float()
            _, recs = _logged(lambda: ops.gemm(A, B, M, N, R, out=out, ldc=N + 8, accumulate=True, rowsum_out=rs, tile=tile, **kw))
            assert recs == [(tile, 1, 1)], recs
            what = "cfg %d %dx%d R=%d" % (tile, M, N, R)
            _assert_bits(out[:M, :N], GR.f32(ref + pre), what)
            _assert_bits(rs[:M], rs_ref, what + ": rowsum_out")
            assert bool((rs[M:] == SENT).all()), what + ": rowsum_out written past M"
            _assert_canary(out, M, N, what)


def _group_problems(mode, seed):
    """Up to 8 problems of one grouped launch: weight gradients (ta + tb, accumulate, row sums on every other one) or forward / data
    gradients (nt / tb) with full epilogues; each with its exact result and canvases."""
    if mode == "wgrad":
        shapes = [(264, 200, 192), (128, 64, 64), (520, 136, 1088), (104, 776, 192), (200, 128, 3072), (136, 1032, 128), (1024, 512, 192),
                  (776, 264, 640)]
    else:
        shapes = [(257, 200, 192), (1600, 264, 768), (130, 1032, 128), (1023, 72, 3072), (300, 520, 64)]
    probs, checks = [], []
    for i, (M, N, K) in enumerate(shapes):
        s = seed + 10 * i
        if mode == "wgrad":
            A, B, kw, acc, pre, rs_pre, rs_ref = _wgrad_rowsum_case(M, N, K, s)
            out = _canvas(M, N, N + 8, torch.float32, inner=pre)
            d = dict(A=A, B=B, M=M, N=N, K=K, out=out, ldc=N + 8, accumulate=True, **kw)
            rs = None
            if i % 2 == 0:
                rs = torch.full((M + 8,), SENT, device=DEV)
                rs[:M] = rs_pre.float()
                d["rowsum_out"] = rs
            probs.append(d)
            checks.append((out, GR.f32(acc + pre), None, None, rs, rs_ref))
            continue
        A, B, kw, acc = _operands(mode, M, N, K, 24, 24, seed=s, extra=1 << 14)
        unit = 2.0 ** -8
        bias = GR.unit_ints((N,), 255, s + 1, unit).to(DEV)
        p = (0.5, 0.75, 0.0)[i % 3]
        keep = host_keep(DROP_SEEDS[1], 30 + i, M, N, p) if p else None
        f32_out = i % 2 == 1
        add = GR.unit_ints((M, N), 255, s + 2, unit * 2).to(DEV)
        out = _canvas(M, N, N + 24, torch.float32 if f32_out else torch.bfloat16)
        pre = _canvas(M, N, N + 8, torch.bfloat16)
        d = dict(A=A, B=B, M=M, N=N, K=K, out=out, ldc=N + 24, bias=bias.float(), act="relu" if i % 2 else "none", preact_out=pre,
                 ld_aux=N + 8, addend=add.float() if f32_out else bf(add), p_drop=p, site=30 + i, seed=DROP_SEEDS[1], **kw)
        r = GR.epilogue(acc, bias=bias, act=d["act"], keep=keep, drop_scale=1.0 / (1.0 - p), addend=add, out="f32" if f32_out else "bf16")
        probs.append(d)
        checks.append((out, r["y"], pre, r["pre"], None, None))
    return probs, checks


@pytest.mark.parametrize("mode", ["wgrad", "nt", "tb"])
@pytest.mark.parametrize("tile", (4, 9))
def test_gemm_grouped_bit_for_bit(mode, tile, gemm_path):
    """crct_gemm_bf16_grouped with up to 8 problems (GROUP_MAX) on both grouped configurations: weight gradients (+ row sums) and forward
    / data-gradient groups with full epilogues; also with crct_gemm_group_target_workgroups at 1 and 7, so that each workgroup walks the
    tiles of several problems.  Every problem against its exact result, not only against its single launch.  On the register-staged
    kernel (gemm_path) the group runs as single launches, without row sums."""
    lib = L.load()
    for target in (0, 1, 7):
        probs, checks = _group_problems(mode, seed=100 * tile + target)
        for d in probs:
            d["tile"] = tile
            if gemm_path == "generic":
                d.pop("rowsum_out", None)
        old = lib.crct_gemm_group_target_workgroups(target)
        try:
            _, recs = _logged(lambda: ops.gemm_grouped(probs))
        finally:
            lib.crct_gemm_group_target_workgroups(old)
        if gemm_path == "pipelined":
            assert recs == [(tile, 1, len(probs))], recs
        else:
            assert recs == [(_ran_cfg(gemm_path, tile, d["M"], d["N"], d["K"]), 1, 1) for d in probs], recs
        for i, ((out, ref, pre, pre_ref, rs, rs_ref), d) in enumerate(zip(checks, probs)):
            what = "%s cfg %d target %d problem %d" % (mode, tile, target, i)
            M, N = d["M"], d["N"]
            _assert_bits(out[:M, :N], ref, what)
            _assert_canary(out, M, N, what)
            if pre is not None:
                _assert_bits(pre[:M, :N], pre_ref, what + ": preact_out")
                _assert_canary(pre, M, N, what + ": preact_out")
            if rs is not None and gemm_path == "pipelined":
                _assert_bits(rs[:M], rs_ref, what + ": rowsum_out")
                assert bool((rs[M:] == SENT).all()), what + ": rowsum_out written past M"


def _stamped_cases():
    """(name, force_generic, run, [(canvas, M, N, exact result)]) of the four launch forms: single LDS-DMA, split-K, grouped, register-staged."""
    def single(name, K, generic, **kw_extra):
        A, B, kw, ref = _operands("nt", 128, 128, K, 48, 48, seed=K)
        buf = _canvas(128, 128, 128 + 24, torch.float32)
        return (name, generic, lambda: ops.gemm(A, B, 128, 128, K, out=buf, ldc=128 + 24, **dict(kw, **kw_extra)), [(buf, 128, 128, GR.f32(ref))])
    probs, outs = [], []
    for i in range(2):
        A, B, kw, ref = _operands("tt", 128, 128, 128, 32, 32, seed=31 + i)
        buf = _canvas(128, 128, 128 + 8, torch.float32)
        probs.append(dict(A=A, B=B, M=128, N=128, K=128, out=buf, ldc=128 + 8, **kw))
        outs.append((buf, 128, 128, GR.f32(ref)))
    return [single("lds-dma", 128, 0), single("split-k", 256, 0, tile=4, split_k=2), ("grouped", 0, lambda: ops.gemm_grouped(probs), outs),
            single("register-staged", 72, 1)]


@pytest.mark.parametrize("gemm_path", ["pipelined"], indirect=True)      # the cases choose the kernel themselves
def test_gemm_stamped_launch_path_same_bits_one_timed_launch(gemm_path):
    """crct_prof_enable(1) sends every GEMM launch through hipExtLaunchKernelGGL with an event pair (only bench.py arms it).  Each launch
    form -- single, split-K on configuration 4 (96 KB of LDS), grouped weight gradients, register-staged -- writes the same bits stamped
    as plain (the exact ones, inside its sentinel canvas), and crct_prof_read then holds exactly one launch: under the variant the
    launch log names (cfg * 3 + kind), with a time above zero."""
    lib = L.load()
    try:
        for name, generic, run, outs in _stamped_cases():
            lib.crct_gemm_force_generic(generic)
            lib.crct_prof_enable(0)
            run()
            plain = [buf.clone() for buf, *_ in outs]
            for buf, *_ in outs:
                buf.fill_(SENT)
            lib.crct_prof_reset()
            lib.crct_prof_enable(1)
            lib.crct_launch_log_enable(1)
            run()
            lib.crct_prof_enable(0)
            assert lib.crct_launch_log_count() == 1, (name, lib.crct_launch_log_count())
            rec = L.LaunchRec()
            assert lib.crct_launch_log_read(0, C.byref(rec)) == 0
            lib.crct_launch_log_enable(0)
            assert (rec.split_k, rec.n_problems) == ((2 if name == "split-k" else 1), len(outs)), (name, rec.cfg, rec.split_k, rec.n_problems)
            assert (rec.cfg >= 16) == bool(generic) and (name != "split-k" or rec.cfg == 4), (name, rec.cfg)
            for (buf, M, N, ref), before in zip(outs, plain):
                assert torch.equal(buf, before), name + ": stamped and plain launches differ"
                _assert_bits(buf[:M, :N], ref, name)
                _assert_canary(buf, M, N, name)
            seen = {}
            for v in range(225):
                cnt, fl, ms = C.c_long(0), C.c_double(0), C.c_double(0)
                assert lib.crct_prof_read(v, C.byref(cnt), C.byref(fl), C.byref(ms)) == 0
                if cnt.value:
                    seen[v] = (cnt.value, ms.value)
            print("%s: launch log cfg %d kind %d, profile %r" % (name, rec.cfg, rec.kind, seen))
            assert list(seen) == [rec.cfg * 3 + rec.kind] and seen[rec.cfg * 3 + rec.kind][0] == 1, (name, rec.cfg, rec.kind, seen)
            assert seen[rec.cfg * 3 + rec.kind][1] > 0, (name, seen)
    finally:
        lib.crct_launch_log_enable(0)
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()
        lib.crct_gemm_force_generic(0)


def test_gemm_refuses_c_cached_with_accumulate(gemm_path):
    """c_cached is a plain fp32 store: the LDS-DMA epilogue writes it without reading the old value, the register-staged one added it.
    The combination is refused by crct_gemm_bf16 and crct_gemm_bf16_grouped on both kernel paths, and nothing is written."""
    for K in (64, 72):             # LDS-DMA kernel (unless gemm_path forces the other) and register-staged kernel
        A, B, kw, _ = _operands("nt", 130, 64, K, 8, 8, seed=K)
        out = torch.full((130, 64), 3.0, device=DEV)
        with pytest.raises(RuntimeError, match="c_cached with accumulate"):
            ops.gemm(A, B, 130, 64, K, out=out, accumulate=True, c_cached=True, **kw)
        other = dict(A=A, B=B, M=130, N=64, K=K, out=torch.zeros(130, 64, device=DEV), **kw)
        with pytest.raises(RuntimeError, match="c_cached with accumulate"):
            ops.gemm_grouped([other, dict(other, out=out, accumulate=True, c_cached=True)])
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and bool((other["out"] == 0).all())
        ops.gemm(A, B, 130, 64, K, out=out, c_cached=True, **kw)          # each flag alone is fine
        ops.gemm(A, B, 130, 64, K, out=out, accumulate=True, **kw)


# ------------------------------------------------------------------------------------------- fp8 GEMMs bit for bit against fp64
def _f8(x, kind):
    return x.float().to(torch.float8_e4m3fn if kind == "e4m3" else torch.float8_e5m2).to(DEV)


@pytest.mark.parametrize("M,N,K,cfg", [(257, 520, 384, 20), (300, 1000, 2048, 21), (130, 1032, 2048, 20), (1600, 768, 3072, 21)])
def test_gemm_fp8_forward_bit_for_bit(M, N, K, cfg):
    """e4m3 integers 1 .. 16 (either sign), power-of-two scales: alpha = 1 / (sa sb) is exact, every sum below 2^20 is exact.  bias, relu,
    preact_out, the e4m3 copy (q_out = _q8 of the exact value) and its amax (exactly max |value|), bf16 and fp32 outputs; ids 20 and 21
    by shape (21: N <= 1024 with K >= 2048)."""
    amax = 16 if K <= 2048 else 8
    qa, qb = GR.operands(M, N, K, amax, amax, seed=M + K, kind="e4m3", extra=1 << 16)
    sa, sb = 8.0, 4.0                                        # q = x * scale: x = q / scale
    acc = GR.ref_nt(qa.to(DEV), qb.to(DEV))                  # in units of 1 / (sa sb)
    bias = GR.unit_ints((N,), 255, 5, 1.0 / 32).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    xa, xb = _f8(qa, "e4m3"), _f8(qb, "e4m3")
    for out_f32 in (True, False):
        pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
        qs = torch.tensor([0.25], device=DEV)
        am = torch.zeros(L.FP8_AMAX_LANES, device=DEV)
        y, recs = _logged(lambda: ops.gemm_fp8(xa, xb, sa_d, sb_d, M, N, K, bias=bias.float(), act="relu", preact_out=pre, out_f32=out_f32,
                                               q_out=q_out, q_scale=qs, q_amax=am))
        assert recs == [(cfg, 1, 1)], recs
        r = GR.epilogue(acc, alpha=1.0 / (sa * sb), bias=bias, act="relu", out="f32" if out_f32 else "bf16", q_scale=0.25, q_kind="e4m3")
        what = "fp8 fwd %dx%dx%d" % (M, N, K)
        _assert_bits(y, r["y"], what)
        _assert_bits(pre, r["pre"], what + ": preact_out")
        _assert_bits(q_out.view(torch.float8_e4m3fn).double(), r["q"], what + ": q_out")
        assert float(am.max()) == r["amax"], what + ": amax"


@pytest.mark.parametrize("M,N,K,cfg", [(257, 264, 1024, 20), (300, 520, 2048, 21)])
def test_gemm_fp8_data_gradient_bit_for_bit(M, N, K, cfg):
    """e5m2 A (integers 1 .. 8) x e4m3 B, dact relu (an exact 0 / 1 factor), the e5m2 q_out copy and its amax."""
    qa, qb = GR.operands(M, N, K, 8, 16, seed=M + N, kind="e5m2", kind_b="e4m3")
    sa, sb = 2.0, 16.0
    acc = GR.ref_nt(qa.to(DEV), qb.to(DEV))
    src = GR.unit_ints((M, N), 8, 9, 1.0).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    qs = torch.tensor([4.0], device=DEV)
    am = torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    y, recs = _logged(lambda: ops.gemm_fp8(_f8(qa, "e5m2"), _f8(qb, "e4m3"), sa_d, sb_d, M, N, K, a_bf8=True, q_bf8=True, dact_src=bf(src),
                                           dact="relu", q_out=q_out, q_scale=qs, q_amax=am))
    assert recs == [(cfg, 1, 1)], recs
    r = GR.epilogue(acc, alpha=1.0 / (sa * sb), dact="relu", dact_src=src, q_scale=4.0, q_kind="e5m2")
    what = "fp8 dgrad %dx%dx%d" % (M, N, K)
    _assert_bits(y, r["y"], what)
    _assert_bits(q_out.view(torch.float8_e5m2).double(), r["q"], what + ": q_out")
    assert float(am.max()) == r["amax"], what + ": amax"


@pytest.mark.parametrize("tile", (36, 37))
def test_gemm_fp8_weight_gradient_bit_for_bit(tile):
    """dW = dy^T x from token-major e5m2 dy (1 .. 8) and e4m3 x (1 .. 16): R not a multiple of 128, N and K multiples of 16 but not of
    the tile, overwrite and accumulate; then grouped launches of 8 problems."""
    sd, sx = 4.0, 8.0
    sd_d, sx_d = torch.tensor([sd], device=DEV), torch.tensor([sx], device=DEV)
    for R in (1, 16, 100, 129, 2880):
        N, K = 144, 208
        GR.check_exact(R, 8, 16, 1 << 12, "e5m2")
        dq, xq = GR.ints((R, N), 8, R, "e5m2"), GR.ints((R, K), 16, R + 3, "e4m3")
        ref = GR.ref_tt(dq.to(DEV), xq.to(DEV)) / (sd * sx)
        pre = GR.unit_ints((N, K), 64, R + 4, 1.0 / 32).to(DEV)
        out = torch.full((N, K), 7.0, device=DEV)
        _, recs = _logged(lambda: ops.gemm_wgrad_fp8([(_f8(dq, "e5m2"), _f8(xq, "e4m3"), sd_d, sx_d, out)], accumulate=False, tile=tile))
        assert recs == [(tile, 1, 1)], recs
        _assert_bits(out, GR.f32(ref), "fp8 wgrad R=%d" % R)
        out = pre.float().clone()
        ops.gemm_wgrad_fp8([(_f8(dq, "e5m2"), _f8(xq, "e4m3"), sd_d, sx_d, out)], accumulate=True, tile=tile)
        _assert_bits(out, GR.f32(ref + pre), "fp8 wgrad accumulate R=%d" % R)
    R = 129
    probs, refs = [], []
    for i, (N, K) in enumerate(((144, 208), (16, 16), (768, 3072), (3072, 768), (272, 48), (64, 1040), (1024, 1024), (48, 336))):
        dq = GR.ints((R, N), 8, 50 + i, "e5m2")
        xq = GR.ints((R, K), 16, 60 + i, "e4m3")
        pre = GR.unit_ints((N, K), 64, 70 + i, 1.0 / 32).to(DEV)
        probs.append((_f8(dq, "e5m2"), _f8(xq, "e4m3"), sd_d, sx_d, pre.float().clone()))
        refs.append(GR.f32(GR.ref_tt(dq.to(DEV), xq.to(DEV)) / (sd * sx) + pre))
    _, recs = _logged(lambda: ops.gemm_wgrad_fp8(probs, accumulate=True, tile=tile))
    assert recs == [(tile, 1, 8)], recs
    for i, (p, ref) in enumerate(zip(probs, refs)):
        _assert_bits(p[4], ref, "fp8 grouped wgrad problem %d" % i)


def test_gemm_configuration_ids_serve_their_operand_kind(gemm_path):
    """A configuration id counts only on the operands its row of k_configs serves.  An fp8 id as CrctGemmArgs.tile of a bf16 GEMM (a
    site policy of an fp8 step, in its bf16 calibration pass) runs configuration 12; each fp8 forward id (20, 21) on an fp8 forward
    problem and each fp8 weight-gradient id (36, 37) on an fp8 weight gradient runs itself, whatever the shape would have chosen.
    Every result bit for bit against the exact one."""
    M, N, K = 129, 72, 64
    A, B, kw, ref = _operands("nt", M, N, K, 48, 48, seed=5)
    for tile in (20, 36):
        expect = (12 if gemm_path == "pipelined" else _ran_cfg(gemm_path, tile, M, N, K), 1, 1)
        _run_exact(A, B, M, N, K, dict(kw, tile=tile), ref, expect, "fp8 id %d on a bf16 GEMM" % tile, False)
    M, N, K = 129, 72, 128                 # by shape this problem runs 20
    qa, qb = GR.operands(M, N, K, 16, 16, seed=9, kind="e4m3")
    sa, sb = torch.tensor([8.0], device=DEV), torch.tensor([4.0], device=DEV)
    xa, xb = _f8(qa, "e4m3"), _f8(qb, "e4m3")
    exact = GR.epilogue(GR.ref_nt(qa.to(DEV), qb.to(DEV)), alpha=1.0 / 32, out="f32")["y"]
    for tile in (20, 21):
        out = torch.full((M, N), SENT, device=DEV)
        g = L.GemmArgs()
        g.A, g.B, g.C, g.scale_a, g.scale_b = L.ptr(xa), L.ptr(xb), L.ptr(out), L.ptr(sa), L.ptr(sb)
        g.lda, g.ldb, g.ldc, g.ld_aux, g.ld_add, g.ld_q = K, K, N, N, N, N
        g.M, g.N, g.K, g.c_is_f32, g.tile, g.alpha, g.fp8 = M, N, K, 1, tile, 1.0, 1
        _, recs = _logged(lambda: L.check(L.load().crct_gemm_bf16(C.byref(g), L.current_stream()), "gemm_fp8"))
        assert recs == [(tile, 1, 1)], (tile, recs)
        _assert_bits(out, exact, "fp8 forward under id %d" % tile)
    R, N, K = 130, 48, 80
    dq, xq = GR.ints((R, N), 8, 3, "e5m2"), GR.ints((R, K), 16, 4, "e4m3")
    exact = GR.f32(GR.ref_tt(dq.to(DEV), xq.to(DEV)) / 32)
    for tile in (36, 37):
        out = torch.full((N, K), SENT, device=DEV)
        _, recs = _logged(lambda: ops.gemm_wgrad_fp8([(_f8(dq, "e5m2"), _f8(xq, "e4m3"), sa, sb, out)], accumulate=False, tile=tile))
        assert recs == [(tile, 1, 1)], (tile, recs)
        _assert_bits(out, exact, "fp8 weight gradient under id %d" % tile)


# ------------------------------------------------------------------------------------------- LayerNorm and column sums against fp64
_LN_CASES = [(1, 64), (7, 96), (255, 520), (1600, 768), (9920, 1024), (255, 2048), (7, 2048), (1600, 520), (1, 1024), (9920, 64)]


def _ln_rows(M, H, seed):
    """Rows N(0.3, 2) with row 0 constant (var = 0: y = beta exactly)."""
    x = rand(M, H, scale=2.0, seed=seed) + 0.3
    x[0] = 0.75
    return x


def _check_ln_forward_terms(x, y, mean, rstd, gamma, beta, what):
    """As _check_ln_forward without dropout, y within one bf16 step + 2^-20 of the terms the kernel combined: gamma (x - mean) rstd is
    formed from x and mean (fp32 each), so where y cancels to near 0 the roundings of |x| rstd and |mean| rstd remain."""
    xd = x.double().cpu()
    m64, sd64, r64 = _ln_stats64(xd)
    assert float(((mean.double().cpu() - m64).abs() / (m64.abs() + sd64)).max()) <= 1e-5, what + ": mean"
    assert float(((rstd.double().cpu() - r64).abs() / r64).max()) <= 1e-5, what + ": rstd"
    g, b = gamma.double().cpu(), beta.double().cpu()
    ref = g * ((xd - m64[:, None]) * r64[:, None]) + b
    scale = g.abs() * (xd.abs() + m64.abs()[:, None]) * r64[:, None] + b.abs()
    _assert_within_bf16_step(y, ref, scale, what + ": y")


def _ln_check_backward(x, dy, mean, rstd, gamma, keep_post, p_post, keep_lin, p_lin, out, what, pre=None):
    """dx (and dx_lin) per element within one bf16 step of fp64 autograd at x, fed dy * keep / (1 - p); dgamma / dbeta / dbias by
    _assert_sums (pre: the accumulated-onto values)."""
    dx, dxl, dg, db, dbias = out
    ks = keep_post.double().cpu() / (1 - p_post) if keep_post is not None else torch.ones(x.shape, dtype=torch.float64)
    ds, dg64, db64, dg_mag, db_mag = _ln_backward64(x, dy, ks, gamma)
    # magnitude of the terms behind dx: rstd * (|g dy'| + mean |g dy'| + |xhat| mean |g dy' xhat|)
    xd = x.double().cpu()
    m64, _, r64 = _ln_stats64(xd)
    xn = (xd - m64[:, None]) * r64[:, None]
    gdy = gamma.double().cpu() * dy.double().cpu() * ks
    mag = r64[:, None] * (gdy.abs() + gdy.abs().mean(1, keepdim=True) + xn.abs() * (gdy * xn).abs().mean(1, keepdim=True))
    _assert_within_bf16_step(dx, ds, mag, what + ": dx")
    lin = ds
    if keep_lin is not None:
        lin = ds * keep_lin.double().cpu() / (1 - p_lin)
        _assert_within_bf16_step(dxl, lin, mag / (1 - p_lin), what + ": dx_lin")
    z = torch.zeros_like(dg64) if pre is None else pre[0].double().cpu()
    _assert_sums(dg, z + dg64, dg_mag + z.abs(), what + ": dgamma")
    z = torch.zeros_like(db64) if pre is None else pre[1].double().cpu()
    _assert_sums(db, z + db64, db_mag + z.abs(), what + ": dbeta")
    z = torch.zeros_like(db64) if pre is None else pre[2].double().cpu()
    _assert_sums(dbias, z + lin.sum(0), (mag * (lin.abs() > 0)).sum(0) + lin.abs().sum(0) + z.abs(), what + ": dbias")


@pytest.mark.parametrize("M,H", _LN_CASES)
def test_layernorm_against_fp64(M, H, gemm_path):
    """crct_layernorm_fwd / _fwd_args (bf16 and fp32 rows, with and without the y_f32 copy) and crct_layernorm_bwd / _bwd_rows_args +
    finalize, per element against fp64: H up to 2048 (520: not a multiple of 64), M over the block counts of crct_layernorm_bwd_blocks
    (the dgamma / dbeta / dbias partials reduced across blocks), constant rows, post- and lin-dropout masks, accumulate.  LayerNorm
    does not go through a GEMM: the register-staged parametrisation (gemm_path) has nothing to add and returns at once."""
    if gemm_path == "generic":
        return
    x = _ln_rows(M, H, seed=M + H)
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3)
    dy = bf(rand(M, H, seed=4))
    for xin in (bf(x), x):
        kind = "bf16" if xin.dtype == torch.bfloat16 else "fp32"
        for y32 in (False, True):
            res = ops.layernorm_fwd(xin, gamma, beta, y_f32=y32)
            y, mean, rstd = res[:3]
            what = "%dx%d %s rows%s" % (M, H, kind, " + y_f32" if y32 else "")
            _check_ln_forward_terms(xin, y, mean, rstd, gamma, beta, what)
            assert bool((y[0] == bf(beta)).all()), what + ": a constant row is beta"
            if y32:
                y32v = res[3]
                assert torch.equal(y, y32v.to(torch.bfloat16)), what
                ref = GR.f32(gamma.double() * ((xin.double() - mean.double()[:, None]) * rstd.double()[:, None]) + beta.double())
                err = (y32v.double() - ref).abs()
                tol = 2.0 ** -21 * ((gamma.double() * (xin.double() - mean.double()[:, None]) * rstd.double()[:, None]).abs() + beta.double().abs())
                assert bool((err <= tol + 2.0 ** -22 * ref.abs()).all()), what + ": y_f32 beyond fp32 rounding of the kernel's own statistics"
        out = ops.layernorm_bwd(dy, xin, mean, rstd, gamma)
        _ln_check_backward(xin, dy, mean, rstd, gamma, None, 0.0, None, 0.0, out, "%dx%d %s bwd" % (M, H, kind))
        # post-norm (p = 0.5) and lin (p = 0.1) dropout, accumulate onto prefilled column sums
        pre = [rand(H, seed=s) for s in (7, 8, 9)]
        seed = DROP_SEEDS[1]
        out = ops.layernorm_bwd(dy, xin, mean, rstd, gamma, want_lin=True, p_lin=0.1, lin_site=19, p_post=0.5, post_site=2, seed=seed,
                                dgamma=pre[0].clone(), dbeta=pre[1].clone(), dbias=pre[2].clone(), accumulate=True)
        _ln_check_backward(xin, dy, mean, rstd, gamma, host_keep(seed, 2, M, H, 0.5), 0.5, host_keep(seed, 19, M, H, 0.1), 0.1, out,
                           "%dx%d %s bwd dropout accumulate" % (M, H, kind), pre=pre)


def test_layernorm_fp32_rows_with_a_large_mean(gemm_path):
    """fp32 rows of mean 1e3 and standard deviation 1e-2 (a pre-LayerNorm sum far from zero): the statistics must hold up to the fp64
    ones (a one-pass E[x^2] - E[x]^2 variance loses every digit here)."""
    if gemm_path == "generic":
        return
    M, H = 255, 768
    x = rand(M, H, scale=1e-2, seed=31) + 1e3
    mean, rstd = ops.layernorm_fwd(x, torch.ones(H, device=DEV), torch.zeros(H, device=DEV))[1:3]
    m64, _, r64 = _ln_stats64(x.double().cpu())
    assert float(((mean.double().cpu() - m64).abs() / (m64.abs() + 1e-2)).max()) <= 1e-5
    assert float(((rstd.double().cpu() - r64).abs() / r64).max()) <= 1e-3, "rstd of a large-mean row"


@pytest.mark.parametrize("M,N,ld", [(1, 64, 64), (255, 520, 528), (1600, 3072, 3072), (9920, 768, 776), (7, 8, 16)])
def test_colsum_on_integers_is_exact(M, N, ld, gemm_path):
    """crct_colsum_bf16 on integer-valued bf16 rows (ld > N: the columns past N are never read), written and accumulated: exact."""
    if gemm_path == "generic":
        return
    x = GR.strided(GR.ints((M, N), 255, M + N).to(DEV), ld, fill=SENT)
    xb = bf(x)
    ref = x[:, :N].sum(0)
    out = ops.colsum(xb, M, N, ld=ld)
    _assert_bits(out, ref, "colsum %dx%d" % (M, N))
    pre = GR.ints((N,), 255, 3).to(DEV)
    out = pre.float().clone()
    ops.colsum(xb, M, N, ld=ld, out=out, accumulate=True)
    _assert_bits(out, ref + pre, "colsum accumulate %dx%d" % (M, N))
