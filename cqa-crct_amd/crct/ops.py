"""Thin torch-tensor wrappers over the kernel launchers of libcrct_hip.so.

torch is used only for device memory and the current HIP stream; every computation below is one
C-ABI call into the hand-written gfx950 kernels (include/crct_hip.h).  bf16 tensors are passed as
``torch.bfloat16``; all tensors must be contiguous CUDA tensors.  These wrappers exist for the kernel
parity tests and for building blocks outside the step engine; the training step itself goes
through ``crct.engine`` (one native call per forward / backward).
"""
import ctypes as C

import torch

from . import lib as L

ACT = dict(none=0, gelu=1, relu=2, leaky=3, tanh=4)


def _chk(t, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libcrct_hip kernels need CUDA (HIP) tensors; got a %s tensor -- no CPU fallback" % t.device)
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError("expected %s, got %s" % (dtype, t.dtype))
    return t


def _drop(p, site):
    thr = L.drop_threshold(p)
    return thr, (1.0 / (1.0 - p) if thr else 1.0), int(site)


def _gemm_args(g, A, B, M, N, K, ta=False, tb=False, lda=None, ldb=None, out=None, ldc=None, bias=None, act="none",
               preact_out=None, dact_src=None, dact="none", ld_aux=None, addend=None, ld_add=None, out_f32=False,
               accumulate=False, tile=-1, alpha=1.0, p_drop=0.0, site=0, seed=0, rowsum_out=None, split_k=0, model_site=0, c_cached=False):
    """addend may be bf16 or fp32 (the fp32 residual stream: CrctGemmArgs.addend_f32); c_cached: an fp32 output that the next kernel
    reads (ordinary instead of streaming stores)."""
    _chk(A, torch.bfloat16), _chk(B, torch.bfloat16)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    g.A, g.B, g.C = L.ptr(A), L.ptr(B), L.ptr(out)
    g.bias, g.preact_out, g.dact_src, g.addend = L.ptr(bias), L.ptr(preact_out), L.ptr(dact_src), L.ptr(addend)
    g.lda = lda if lda is not None else (M if ta else K)
    g.ldb = ldb if ldb is not None else (N if tb else K)
    g.ldc = ldc if ldc is not None else N
    g.ld_aux = ld_aux if ld_aux is not None else N
    g.ld_add = ld_add if ld_add is not None else N
    g.M, g.N, g.K, g.ta, g.tb = M, N, K, int(ta), int(tb)
    g.act, g.dact, g.c_is_f32, g.accumulate, g.tile, g.alpha = ACT[act], ACT[dact], int(out.dtype == torch.float32), int(accumulate), tile, alpha
    g.drop_thr, g.drop_scale, g.drop_site = _drop(p_drop, site)
    g.seed = seed
    g.rowsum_out = L.ptr(rowsum_out)
    g.site = int(model_site)
    g.addend_f32 = int(addend is not None and addend.dtype == torch.float32)
    g.c_cached = int(bool(c_cached))
    if split_k and split_k > 1:       # K-partitioned launch: slab space + ticket words (zero before the first use) per device
        ws, cnt = _splitk_space(A.device, M, N, split_k)
        g.split_k, g.splitk_ws, g.splitk_cnt = int(split_k), L.ptr(ws), L.ptr(cnt)
        g._keep = (ws, cnt)
    return out


_SPLITK = {}


def _splitk_space(dev, M, N, S):
    lib = L.load()
    need, tickets = lib.crct_gemm_splitk_ws_elems(M, N, S), lib.crct_gemm_splitk_tickets(M, N)
    ws, cnt = _SPLITK.get(dev, (None, None))
    if ws is None or ws.numel() < need or cnt.numel() < tickets:
        ws = torch.empty(max(need, ws.numel() if ws is not None else 0), dtype=torch.float32, device=dev)
        cnt = torch.zeros(max(tickets, 4096), dtype=torch.int32, device=dev)
        _SPLITK[dev] = (ws, cnt)
    return ws, cnt


def _ln_addend(ln, src):
    """``src`` = (mean [M], rstd [M], gamma [N], beta [N]), fp32: CrctGemmLnAddend (None: no LayerNorm addend)."""
    if src is not None:
        for t in src:
            _chk(t, torch.float32)
        ln.mean, ln.rstd, ln.gamma, ln.beta = (L.ptr(t) for t in src)
    return ln


def gemm(A, B, M, N, K, ln_addend=None, **kw):
    """One GEMM with its fused epilogue (keyword arguments: see ``_gemm_args``).  ln_addend = (mean, rstd, gamma, beta): the fp32
    ``addend`` holds the rows a LayerNorm normalised and the epilogue adds that LayerNorm's fp32 output, rebuilt per element
    (crct_gemm_bf16_ln_addend) -- the bits of ``layernorm_fwd(..., y_f32=True)``'s fp32 output as a plain fp32 addend."""
    g = L.GemmArgs()
    out = _gemm_args(g, A, B, M, N, K, **kw)
    if ln_addend is not None:
        ln = _ln_addend(L.GemmLnAddend(), ln_addend)
        L.check(L.load().crct_gemm_bf16_ln_addend(C.byref(g), C.byref(ln), L.current_stream()), "gemm (LayerNorm addend)")
        return out
    L.check(L.load().crct_gemm_bf16(C.byref(g), L.current_stream()), "gemm")
    return out


def gemm_grouped(problems):
    """``problems`` = [dict(A=, B=, M=, N=, K=, ...gemm keywords)] sharing (ta, tb): ONE grouped launch (crct_gemm_bf16_grouped),
    every problem with its own epilogue.  Returns the outputs."""
    arr = (L.GemmArgs * len(problems))()
    lns = (L.GemmLnAddend * len(problems))()
    srcs = [prob.get("ln_addend") for prob in problems]
    outs = [_gemm_args(g, **{k: v for k, v in prob.items() if k != "ln_addend"}) for g, prob in zip(arr, problems)]
    if any(src is not None for src in srcs):      # a problem's ``ln_addend``: as for ``gemm``
        for ln, src in zip(lns, srcs):
            _ln_addend(ln, src)
        L.check(L.load().crct_gemm_bf16_grouped_ln_addend(arr, lns, len(problems), L.current_stream()), "gemm_grouped (LayerNorm addend)")
        return outs
    L.check(L.load().crct_gemm_bf16_grouped(arr, len(problems), L.current_stream()), "gemm_grouped")
    return outs


def gemm_fp8(Aq, Bq, scale_a, scale_b, M, N, K, bias=None, act="none", preact_out=None, addend=None, p_drop=0.0, site=0, seed=0,
             out_f32=False, q_out=None, q_scale=None, q_amax=None, a_bf8=False, q_bf8=False, dact_src=None, dact="none"):
    """y = act((Aq / sa) (Bq / sb)^T + bias) from OCP e4m3 operands (uint8 / float8_e4m3fn tensors [M][K], [N][K]); scale_* are
    device fp32 scalars.  q_out: e4m3 copy of y quantised with q_scale, max |y| max-ed into q_amax.  a_bf8: Aq holds OCP e5m2
    (a gradient: the fp8 data-gradient GEMMs); q_bf8: the q_out copy is e5m2."""
    lib = L.load()
    out = torch.empty(M, N, device=Aq.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    g = L.GemmArgs()
    g.A, g.B, g.C = L.ptr(Aq), L.ptr(Bq), L.ptr(out)
    g.bias, g.preact_out, g.addend = L.ptr(bias), L.ptr(preact_out), L.ptr(addend)
    g.lda, g.ldb, g.ldc, g.ld_aux, g.ld_add = K, K, N, N, N
    g.M, g.N, g.K = M, N, K
    g.act, g.c_is_f32, g.tile, g.alpha = ACT[act], int(out_f32), -1, 1.0
    g.drop_thr, g.drop_scale, g.drop_site = _drop(p_drop, site)
    g.seed = seed
    g.dact_src, g.dact = L.ptr(dact_src), ACT[dact]
    g.fp8, g.scale_a, g.scale_b = 1 | (2 if a_bf8 else 0) | (4 if q_bf8 else 0), L.ptr(scale_a), L.ptr(scale_b)
    g.q_out, g.q_scale, g.q_amax, g.ld_q = L.ptr(q_out), L.ptr(q_scale), L.ptr(q_amax), N
    L.check(lib.crct_gemm_bf16(C.byref(g), L.current_stream()), "gemm_fp8")
    return out


def gemm_wgrad_grouped(problems):
    """``problems`` = [(dy[R][N], x[R][K], out[N][K] fp32[, db[N] fp32])]: out += dy^T x (db += colsum dy), ONE launch."""
    lib = L.load()
    arr = (L.GemmArgs * len(problems))()
    for g, prob in zip(arr, problems):
        dy, x, out = prob[:3]
        g.rowsum_out = L.ptr(prob[3]) if len(prob) > 3 else None      # optional bias gradient [N] += column sums of dy
        _chk(dy, torch.bfloat16), _chk(x, torch.bfloat16), _chk(out, torch.float32)
        R, N = dy.shape
        K = x.shape[1]
        g.A, g.B, g.C = L.ptr(dy), L.ptr(x), L.ptr(out)
        g.lda, g.ldb, g.ldc, g.ld_aux, g.ld_add = N, K, K, K, K
        g.M, g.N, g.K, g.ta, g.tb = N, K, R, 1, 1
        g.c_is_f32, g.accumulate, g.tile, g.alpha = 1, 1, -1, 1.0
    L.check(lib.crct_gemm_bf16_grouped(arr, len(problems), L.current_stream()), "gemm_grouped")


def gemm_wgrad_fp8(problems, accumulate=True, tile=-1):
    """fp8 weight gradients: ``problems`` = [(dyq[R][N] e5m2, xq[R][K] e4m3, scale_dy, scale_x, out[N][K] fp32)]:
    out (+)= (dyq / s_dy)^T (xq / s_x) with fp32 accumulation; one launch for two or more problems, R (tokens) arbitrary,
    N and K multiples of 16."""
    lib = L.load()
    arr = (L.GemmArgs * len(problems))()
    for g, (dyq, xq, s_dy, s_x, out) in zip(arr, problems):
        _chk(out, torch.float32)
        R, N = dyq.shape
        K = xq.shape[1]
        assert xq.shape[0] == R and out.shape == (N, K) and dyq.element_size() == 1 and xq.element_size() == 1
        g.A, g.B, g.C = L.ptr(dyq), L.ptr(xq), L.ptr(out)
        g.lda, g.ldb, g.ldc, g.ld_aux, g.ld_add = N, K, K, K, K
        g.M, g.N, g.K, g.ta, g.tb = N, K, R, 1, 1
        g.c_is_f32, g.accumulate, g.tile, g.alpha = 1, int(accumulate), tile, 1.0
        g.fp8, g.scale_a, g.scale_b = 1 | 2, L.ptr(s_dy), L.ptr(s_x)
    if len(problems) == 1:
        L.check(lib.crct_gemm_bf16(C.byref(arr[0]), L.current_stream()), "gemm_wgrad_fp8")
    else:
        L.check(lib.crct_gemm_bf16_grouped(arr, len(problems), L.current_stream()), "gemm_wgrad_fp8 (grouped)")


def layernorm_fwd(x, gamma, beta, eps=1e-12, p_drop=0.0, site=0, seed=0, y_f32=False):
    """x bf16 or fp32 [M, H] (fp32: the pre-LayerNorm sums of the fp32 residual stream); y_f32: also return y as fp32 (4th result)."""
    lib = L.load()
    M, H = x.shape
    y = torch.empty(M, H, device=x.device, dtype=torch.bfloat16)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    thr, sc, st = _drop(p_drop, site)
    if x.dtype == torch.float32 or y_f32:
        y32 = torch.empty(M, H, device=x.device, dtype=torch.float32) if y_f32 else None
        a = L.LnFwdArgs()
        a.x, a.gamma, a.beta, a.y, a.mean, a.rstd = L.ptr(_chk(x)), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd)
        a.M, a.H, a.eps, a.drop_thr, a.drop_scale, a.drop_site, a.seed = M, H, eps, thr, sc, st, seed
        a.x_f32, a.y_f32 = int(x.dtype == torch.float32), L.ptr(y32)
        L.check(lib.crct_layernorm_fwd_args(C.byref(a), L.current_stream()), "layernorm_fwd")
        return (y, mean, rstd, y32) if y_f32 else (y, mean, rstd)
    L.check(lib.crct_layernorm_fwd(L.ptr(_chk(x, torch.bfloat16)), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd),
                                   M, H, eps, thr, sc, st, seed, L.current_stream()), "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, want_lin=False, p_lin=0.0, lin_site=0, p_post=0.0, post_site=0, seed=0,
                  dgamma=None, dbeta=None, dbias=None, accumulate=False):
    lib = L.load()
    M, H = x.shape
    dx = torch.empty_like(dy)
    dxl = torch.empty_like(dy) if want_lin else None
    nb = lib.crct_layernorm_bwd_blocks(M)
    part = torch.empty(3 * 4 * nb * H, device=x.device, dtype=torch.float32)       # one partial row per wave
    dgamma = torch.zeros(H, device=x.device) if dgamma is None else dgamma
    dbeta = torch.zeros(H, device=x.device) if dbeta is None else dbeta
    dbias = torch.zeros(H, device=x.device) if dbias is None else dbias
    pt, ps, psite = _drop(p_post, post_site)
    lt, ls, lsite = _drop(p_lin, lin_site)
    if x.dtype == torch.float32:      # the saved pre-norm rows of the fp32 residual stream: rows pass from the struct, then the column pass
        a = L.LnBwdArgs()
        a.dy, a.x, a.mean, a.rstd, a.gamma, a.dx, a.dx_lin, a.partials = (L.ptr(_chk(dy, torch.bfloat16)), L.ptr(x), L.ptr(mean), L.ptr(rstd),
                                                                            L.ptr(gamma), L.ptr(dx), L.ptr(dxl), L.ptr(part))
        a.M, a.H, a.post_thr, a.post_scale, a.post_site, a.lin_thr, a.lin_scale, a.lin_site, a.seed = M, H, pt, ps, psite, lt, ls, lsite, seed
        a.x_f32 = 1
        L.check(lib.crct_layernorm_bwd_rows_args(C.byref(a), L.current_stream()), "layernorm_bwd")
        L.check(lib.crct_layernorm_bwd_finalize(L.ptr(part), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dbias), M, H, int(accumulate), L.current_stream()),
                "layernorm_bwd (finalize)")
        return dx, dxl, dgamma, dbeta, dbias
    L.check(lib.crct_layernorm_bwd(L.ptr(_chk(dy, torch.bfloat16)), L.ptr(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(dx), L.ptr(dxl),
                                   L.ptr(dgamma), L.ptr(dbeta), L.ptr(dbias), L.ptr(part), M, H, int(accumulate),
                                   pt, ps, psite, lt, ls, lsite, seed, L.current_stream()), "layernorm_bwd")
    return dx, dxl, dgamma, dbeta, dbias


def colsum(x, M, N, ld=None, out=None, accumulate=False):
    lib = L.load()
    nb = lib.crct_colsum_blocks(M)
    part = torch.empty(nb * N, device=x.device, dtype=torch.float32)
    out = torch.zeros(N, device=x.device) if out is None else out
    L.check(lib.crct_colsum_bf16(L.ptr(_chk(x, torch.bfloat16)), ld if ld is not None else N, L.ptr(out), L.ptr(part), M, N,
                                 int(accumulate), L.current_stream()), "colsum")
    return out


def softmax_rows(x):
    """Row softmax of fp32 or bf16 features [M, F] -> bf16 (the step's F.softmax(image_feat), either input type)."""
    lib = L.load()
    M, F = x.shape
    y = torch.empty(M, F, device=x.device, dtype=torch.bfloat16)
    fn = lib.crct_softmax_rows_bf16_bf16 if x.dtype == torch.bfloat16 else lib.crct_softmax_rows_f32_bf16
    L.check(fn(L.ptr(_chk(x, x.dtype if x.dtype == torch.bfloat16 else torch.float32)), L.ptr(y), M, F, L.current_stream()), "softmax_rows")
    return y


def softmax_bwd_rows(x, g):
    """Gradient of the row softmax with respect to fp32 or bf16 features x [M, F] for the upstream gradient g (fp32 [M, F]) -> fp32 [M, F]."""
    M, F = x.shape
    dx = torch.empty(M, F, device=x.device, dtype=torch.float32)
    _chk(x, torch.bfloat16 if x.dtype == torch.bfloat16 else torch.float32)
    L.check(L.load().crct_softmax_bwd_rows(L.ptr(x), int(x.dtype == torch.bfloat16), L.ptr(_chk(g, torch.float32)), L.ptr(dx), M, F,
                                           L.current_stream()), "softmax_bwd_rows")
    return dx


def embed_input_grad(dy, sum_saved, mean, rstd, gamma, loc=None, w_loc=None, w_areas=None, want=("d_loc", "d_areas", "d_sum"),
                     p_drop=0.0, site=0, seed=0):
    """Gradients of an embedding's float inputs from its LayerNorm's saved state (crct_embed_input_grad): dy, sum_saved bf16 [M, H];
    ``want`` names the outputs -- (d_loc fp32 [M, 4], d_areas fp32 [M], d_sum fp32 [M, H]), None for the ones left out."""
    M, H = dy.shape
    dev = dy.device
    d_loc = torch.empty(M, 4, device=dev) if "d_loc" in want else None
    d_areas = torch.empty(M, device=dev) if "d_areas" in want else None
    d_sum = torch.empty(M, H, device=dev) if "d_sum" in want else None
    thr, scale, site = _drop(p_drop, site)
    L.check(L.load().crct_embed_input_grad(L.ptr(_chk(dy, torch.bfloat16)), L.ptr(_chk(sum_saved, torch.bfloat16)), L.ptr(_chk(mean, torch.float32)),
                                           L.ptr(_chk(rstd, torch.float32)), L.ptr(_chk(gamma, torch.float32)), L.ptr(_chk(loc, torch.float32)),
                                           L.ptr(_chk(w_loc, torch.float32)), L.ptr(_chk(w_areas, torch.float32)), L.ptr(d_loc), L.ptr(d_areas),
                                           L.ptr(d_sum), M, H, thr, scale, site, int(seed), L.current_stream()), "embed_input_grad")
    return d_loc, d_areas, d_sum


def cast_bf16(x, out=None):
    lib = L.load()
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if out is None else out
    L.check(lib.crct_cast_f32_bf16(L.ptr(_chk(x, torch.float32)), L.ptr(out), x.numel(), L.current_stream()), "cast")
    return out


def _attn_out(t, B, T, Hh, like, what):
    """A caller-supplied attention output: a bf16 [B, T, heads * d] view whose rows (stride(1), the leading dimension the kernel gets)
    may lie in a wider buffer -- batches follow one another (stride(0) = T * stride(1)), columns are contiguous.  None: a fresh
    contiguous tensor."""
    if t is None:
        return torch.empty(B, T, Hh, device=like.device, dtype=torch.bfloat16)
    _chk(t, torch.bfloat16)
    if tuple(t.shape) != (B, T, Hh) or t.stride(2) != 1 or t.stride(1) < Hh or (B > 1 and t.stride(0) != T * t.stride(1)):
        raise RuntimeError("%s: expected a [%d, %d, %d] view with unit column stride and batch stride T * stride(1); got shape %s strides %s"
                           % (what, B, T, Hh, tuple(t.shape), tuple(t.stride())))
    return t


def _attn_outs(outs, B, Tq, Tk, Hh, like, what):
    dq, dk, dv = outs if outs is not None else (None, None, None)
    return (_attn_out(dq, B, Tq, Hh, like, what + ": outs[0] (dq)"), _attn_out(dk, B, Tk, Hh, like, what + ": outs[1] (dk)"),
            _attn_out(dv, B, Tk, Hh, like, what + ": outs[2] (dv)"))


def _q_twin(t):
    """Zeroed uint8 tensor with t's shape and element strides: the fp8 copy shares its bf16 twin's leading dimension (in bytes)."""
    B, T, Hh = t.shape
    return torch.zeros(B * T * t.stride(1), device=t.device, dtype=torch.uint8).as_strided((B, T, Hh), (T * t.stride(1), t.stride(1), 1))


def attention_fwd(q, k, v, keymask, heads, d, p_drop=0.0, site=0, seed=0, row_lse=None, out=None):
    """q [B,Tq,ldq] / k,v [B,Tk,ld*] bf16 (may be column slices of a wider buffer: pass the *slice*).
    row_lse: fp32 [B, heads, Tq] that the long-sequence kernels fill with the softmax row statistics (CrctAttnQuant.row_lse; the
    other kernels leave it untouched) -- hand it, with the returned ctx, to ``attention_bwd``.
    out: ctx goes there, a [B, Tq, heads * d] view that may be a column slice of a wider buffer (its stride(1) is the kernel's ldo)."""
    lib = L.load()
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    ctx = _attn_out(out, B, Tq, heads * d, q, "attention_fwd: out")
    thr, sc, st = _drop(p_drop, site)
    if row_lse is not None:
        assert tuple(row_lse.shape) == (B, heads, Tq)
        qz = L.AttnQuant()
        qz.row_lse = L.ptr(_chk(row_lse, torch.float32))
        L.check(lib.crct_attention_fwd_q(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(_chk(keymask, torch.uint8)), L.ptr(ctx), B, heads, Tq, Tk, d,
                                         q.stride(1), k.stride(1), v.stride(1), ctx.stride(1), thr, sc, st, seed, C.byref(qz), L.current_stream()),
                "attention_fwd")
        return ctx
    L.check(lib.crct_attention_fwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(_chk(keymask, torch.uint8)), L.ptr(ctx), B, heads, Tq, Tk, d,
                                   q.stride(1), k.stride(1), v.stride(1), ctx.stride(1), thr, sc, st, seed, L.current_stream()),
            "attention_fwd")
    return ctx


def attention_probs(q, k, keymask, heads, d, p_drop=0.0, site=0, seed=0, out=None):
    """The attention probabilities of ``attention_fwd`` on the same q / k / keymask, fp32 [B, heads, Tq, Tk] (crct_attention_probs):
    keep / (1 - p) * softmax(q k^T / sqrt(d) + (1 - keymask) * -10000).  q [B,Tq,ldq] / k [B,Tk,ldk] bf16, column slices of wider
    buffers included; with the forward's (p_drop, site, seed) the map carries the dropout mask that forward applied.
    out: a contiguous fp32 tensor of that shape to write into."""
    lib = L.load()
    _chk(q, torch.bfloat16), _chk(k, torch.bfloat16)
    if q.dim() != 3 or k.dim() != 3 or q.shape[0] != k.shape[0] or q.shape[2] != heads * d or k.shape[2] != heads * d:
        raise RuntimeError("attention_probs: q [B, Tq, heads * d] and k [B, Tk, heads * d] expected with heads * d = %d; got %s and %s"
                           % (heads * d, tuple(q.shape), tuple(k.shape)))
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    for t, T, what in ((q, Tq, "q"), (k, Tk, "k")):
        if t.stride(2) != 1 or (B > 1 and t.stride(0) != T * t.stride(1)):
            raise RuntimeError("attention_probs: %s needs unit column stride and batch stride T * stride(1); got strides %s" % (what, tuple(t.stride())))
    _chk(keymask, torch.uint8)
    if tuple(keymask.shape) != (B, Tk) or not keymask.is_contiguous():
        raise RuntimeError("attention_probs: keymask must be a contiguous uint8 [%d, %d]; got %s" % (B, Tk, tuple(keymask.shape)))
    if out is None:
        out = torch.empty(B, heads, Tq, Tk, device=q.device, dtype=torch.float32)
    else:
        _chk(out, torch.float32)
        if tuple(out.shape) != (B, heads, Tq, Tk) or not out.is_contiguous():
            raise RuntimeError("attention_probs: out must be a contiguous fp32 [%d, %d, %d, %d]; got shape %s strides %s"
                               % (B, heads, Tq, Tk, tuple(out.shape), tuple(out.stride())))
    thr, sc, st = _drop(p_drop, site)
    L.check(lib.crct_attention_probs(L.ptr(q), L.ptr(k), L.ptr(keymask), L.ptr(out), B, heads, Tq, Tk, d, q.stride(1), k.stride(1),
                                     thr, sc, st, seed, L.current_stream()), "attention_probs")
    return out


def attention_probs_bwd(q, k, keymask, d_probs, heads, d, outs, accumulate=True, scale=1.0, p_drop=0.0, site=0, seed=0):
    """Backward of the map ``attention_probs`` returns for the same q / k / keymask / (p_drop, site, seed) (crct_attention_probs_bwd):
    with the upstream gradient ``d_probs`` (contiguous fp32 [B, heads, Tq, Tk]) times ``scale`` it adds the map's contribution onto
    ``outs = (dq, dk)`` -- bf16 [B, Tq, lddq] / [B, Tk, lddk] with the column layout of q / k, column slices of wider buffers included --
    or, ``accumulate=False``, writes the contribution alone.  Two launches, bit-reproducible; returns ``outs``."""
    lib = L.load()
    _chk(q, torch.bfloat16), _chk(k, torch.bfloat16)
    if q.dim() != 3 or k.dim() != 3 or q.shape[0] != k.shape[0] or q.shape[2] != heads * d or k.shape[2] != heads * d:
        raise RuntimeError("attention_probs_bwd: q [B, Tq, heads * d] and k [B, Tk, heads * d] expected with heads * d = %d; got %s and %s"
                           % (heads * d, tuple(q.shape), tuple(k.shape)))
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    dq, dk = outs
    _chk(dq, torch.bfloat16), _chk(dk, torch.bfloat16)
    if tuple(dq.shape) != tuple(q.shape) or tuple(dk.shape) != tuple(k.shape):
        raise RuntimeError("attention_probs_bwd: outs = (dq, dk) must have the shapes of q and k; got %s and %s" % (tuple(dq.shape), tuple(dk.shape)))
    for t, T, what in ((q, Tq, "q"), (k, Tk, "k"), (dq, Tq, "dq"), (dk, Tk, "dk")):
        if t.stride(2) != 1 or (B > 1 and t.stride(0) != T * t.stride(1)):
            raise RuntimeError("attention_probs_bwd: %s needs unit column stride and batch stride T * stride(1); got strides %s" % (what, tuple(t.stride())))
    _chk(keymask, torch.uint8)
    if tuple(keymask.shape) != (B, Tk) or not keymask.is_contiguous():
        raise RuntimeError("attention_probs_bwd: keymask must be a contiguous uint8 [%d, %d]; got %s" % (B, Tk, tuple(keymask.shape)))
    _chk(d_probs, torch.float32)
    if tuple(d_probs.shape) != (B, heads, Tq, Tk) or not d_probs.is_contiguous():
        raise RuntimeError("attention_probs_bwd: d_probs must be a contiguous fp32 [%d, %d, %d, %d]; got shape %s strides %s"
                           % (B, heads, Tq, Tk, tuple(d_probs.shape), tuple(d_probs.stride())))
    scratch = torch.empty(max(B * heads * Tq * 3, 1), device=q.device, dtype=torch.float32)      # row statistics: m, 1 / l, delta
    thr, sc, st = _drop(p_drop, site)
    L.check(lib.crct_attention_probs_bwd(L.ptr(q), L.ptr(k), L.ptr(keymask), L.ptr(d_probs), float(scale), L.ptr(dq), L.ptr(dk), L.ptr(scratch),
                                         int(bool(accumulate)), B, heads, Tq, Tk, d, q.stride(1), k.stride(1), dq.stride(1), dk.stride(1),
                                         thr, sc, st, seed, L.current_stream()), "attention_probs_bwd")
    return outs


def attention_fwd_q(q, k, v, keymask, heads, d, q_scale, q_amax, p_drop=0.0, site=0, seed=0, out=None):
    """attention_fwd that also returns the e4m3 copy of ctx (uint8, same shape and strides), quantised with the device scalar q_scale."""
    lib = L.load()
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    ctx = _attn_out(out, B, Tq, heads * d, q, "attention_fwd_q: out")
    ctx_q = _q_twin(ctx)
    qz = L.AttnQuant()
    qz.ctx_q, qz.ctx_scale, qz.ctx_amax = L.ptr(ctx_q), L.ptr(q_scale), L.ptr(q_amax)
    thr, sc, st = _drop(p_drop, site)
    L.check(lib.crct_attention_fwd_q(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(_chk(keymask, torch.uint8)), L.ptr(ctx), B, heads, Tq, Tk, d,
                                     q.stride(1), k.stride(1), v.stride(1), ctx.stride(1), thr, sc, st, seed, C.byref(qz), L.current_stream()),
            "attention_fwd_q")
    return ctx, ctx_q


def attention_bwd_q(q, k, v, keymask, dctx, heads, d, dq_scale, dq_amax, dkv_scale, dkv_amax, p_drop=0.0, site=0, seed=0, row_lse=None,
                    ctx=None, outs=None):
    """attention_bwd that also returns the e5m2 copies of dq, dk, dv (uint8, each with the strides of its bf16 twin); row_lse / ctx / outs
    as in ``attention_bwd``."""
    lib = L.load()
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    dq, dk, dv = _attn_outs(outs, B, Tq, Tk, heads * d, q, "attention_bwd_q")
    dq8, dk8, dv8 = (_q_twin(t) for t in (dq, dk, dv))
    qz = L.AttnQuant()
    qz.dq_q, qz.dk_q, qz.dv_q = L.ptr(dq8), L.ptr(dk8), L.ptr(dv8)
    qz.dq_scale, qz.dq_amax, qz.dkv_scale, qz.dkv_amax = L.ptr(dq_scale), L.ptr(dq_amax), L.ptr(dkv_scale), L.ptr(dkv_amax)
    if row_lse is not None or ctx is not None:
        qz.row_lse, qz.ctx, qz.ld_ctx = L.ptr(_chk(row_lse, torch.float32)), L.ptr(_chk(ctx, torch.bfloat16)), (ctx.stride(1) if ctx is not None else 0)
    thr, sc, st = _drop(p_drop, site)
    L.check(lib.crct_attention_bwd_q(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(keymask), L.ptr(_chk(dctx, torch.bfloat16)), L.ptr(dq), L.ptr(dk), L.ptr(dv),
                                     B, heads, Tq, Tk, d, q.stride(1), k.stride(1), v.stride(1), dctx.stride(1),
                                     dq.stride(1), dk.stride(1), dv.stride(1), thr, sc, st, seed, C.byref(qz), L.current_stream()), "attention_bwd_q")
    return (dq, dk, dv), (dq8, dk8, dv8)


def attention_bwd(q, k, v, keymask, dctx, heads, d, p_drop=0.0, site=0, seed=0, row_lse=None, ctx=None, outs=None):
    """row_lse / ctx: what ``attention_fwd(..., row_lse=)`` of the same operands produced -- the long-sequence kernels then skip
    their statistics sweep (the other kernels ignore both).
    outs: (dq, dk, dv) to write into, [B, Tq | Tk, heads * d] views that may be column slices of wider buffers, as the step engine's
    fused dqkv buffers are (their stride(1) are the kernel's lddq / lddk / lddv)."""
    lib = L.load()
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    dq, dk, dv = _attn_outs(outs, B, Tq, Tk, heads * d, q, "attention_bwd")
    thr, sc, st = _drop(p_drop, site)
    if row_lse is not None or ctx is not None:
        qz = L.AttnQuant()
        qz.row_lse, qz.ctx, qz.ld_ctx = L.ptr(_chk(row_lse, torch.float32)), L.ptr(_chk(ctx, torch.bfloat16)), (ctx.stride(1) if ctx is not None else 0)
        L.check(lib.crct_attention_bwd_q(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(keymask), L.ptr(_chk(dctx, torch.bfloat16)), L.ptr(dq), L.ptr(dk),
                                         L.ptr(dv), B, heads, Tq, Tk, d, q.stride(1), k.stride(1), v.stride(1), dctx.stride(1),
                                         dq.stride(1), dk.stride(1), dv.stride(1), thr, sc, st, seed, C.byref(qz), L.current_stream()), "attention_bwd")
        return dq, dk, dv
    L.check(lib.crct_attention_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(keymask), L.ptr(_chk(dctx, torch.bfloat16)), L.ptr(dq), L.ptr(dk), L.ptr(dv),
                                   B, heads, Tq, Tk, d, q.stride(1), k.stride(1), v.stride(1), dctx.stride(1),
                                   dq.stride(1), dk.stride(1), dv.stride(1), thr, sc, st, seed, L.current_stream()), "attention_bwd")
    return dq, dk, dv


def adamw_plan(seg_len):
    """Host-side block table for crct_adamw_step: returns (blk_seg int32[n], blk_off int64[n])."""
    lib = L.load()
    lens = torch.as_tensor(seg_len, dtype=torch.int64)
    n = lib.crct_adamw_plan(lens.data_ptr(), lens.numel(), None, None, 0)
    blk_seg = torch.empty(n, dtype=torch.int32)
    blk_off = torch.empty(n, dtype=torch.int64)
    lib.crct_adamw_plan(lens.data_ptr(), lens.numel(), blk_seg.data_ptr(), blk_off.data_ptr(), n)
    return blk_seg, blk_off


def grad_sumsq(grads, seg_off, seg_len, blk_seg, blk_off, partials=None, norm_kind=0, max_workgroups=0):
    """crct_grad_sumsq over the chunk table of ``adamw_plan``: ``grads`` is the flat gradient buffer, fp32 or bf16 (the dtype picks
    the source).  Returns partials fp32 [n_blk]: per chunk the sum of squares (norm_kind 0) or max |g| (1, NaN propagating)."""
    if grads.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("grad_sumsq: fp32 or bf16 gradient buffer expected (got %s)" % grads.dtype)
    n_blk = blk_seg.numel()
    if partials is None:
        partials = torch.empty(n_blk, dtype=torch.float32, device=grads.device)
    bf = grads.dtype == torch.bfloat16
    L.check(L.load().crct_grad_sumsq(None if bf else grads.data_ptr(), grads.data_ptr() if bf else None, seg_off.data_ptr(),
                                     seg_len.data_ptr(), blk_seg.data_ptr(), blk_off.data_ptr(), n_blk, _chk(partials, torch.float32).data_ptr(),
                                     int(norm_kind), int(max_workgroups), L.current_stream()), "grad_sumsq")
    return partials


def grad_norm_finalize(partials, blk_seg, n_seg, max_norm, norm_kind=0, grad_scale=None, mul=None, seg_norm=True):
    """crct_grad_norm_finalize: (out fp32 [2] = (norm, clip coefficient), seg_norm fp32 [n_seg] or None), all on the device.
    ``grad_scale`` / ``mul``: optional device fp32 scalars (the norm is divided by the first, the coefficient multiplied by the second)."""
    out = torch.empty(2, dtype=torch.float32, device=partials.device)
    per = torch.empty(n_seg, dtype=torch.float32, device=partials.device) if seg_norm else None
    L.check(L.load().crct_grad_norm_finalize(_chk(partials, torch.float32).data_ptr(), blk_seg.data_ptr(), blk_seg.numel(), int(n_seg),
                                             int(norm_kind), float(max_norm), L.ptr(_chk(grad_scale, torch.float32)),
                                             L.ptr(_chk(mul, torch.float32)), out.data_ptr(), L.ptr(per), L.current_stream()),
            "grad_norm_finalize")
    return out, per


def scale_runs(grads, coef, seg_off, seg_len, blk_seg, blk_off, max_workgroups=0):
    """crct_scale_runs: grads (flat fp32) *= coef (device fp32 scalar) over the chunk table, in place."""
    L.check(L.load().crct_scale_runs(_chk(grads, torch.float32).data_ptr(), _chk(coef, torch.float32).data_ptr(), seg_off.data_ptr(),
                                     seg_len.data_ptr(), blk_seg.data_ptr(), blk_off.data_ptr(), blk_seg.numel(), int(max_workgroups),
                                     L.current_stream()), "scale_runs")
    return grads


def _amp_state(amp):
    """dict(grad_scale=, found_inf=, step=) of device tensors (each optional) -> (CrctAmpState, byref) or (None, None)"""
    if amp is None:
        return None, None
    st = L.AmpState()
    st.grad_scale = L.ptr(_chk(amp.get("grad_scale"), torch.float32))
    st.found_inf = L.ptr(_chk(amp.get("found_inf"), torch.float32))
    st.step = L.ptr(_chk(amp.get("step"), torch.int32))
    return st, C.byref(st)


def _fp8_shadow(fp8):
    """dict(q=, seg_slot=, scale=, amax=[, qt=, seg_in=, seg_t_base=, seg_t_ld=]) of device tensors -> (CrctFp8Shadow, byref)"""
    if fp8 is None:
        return None, None
    sh = L.Fp8Shadow()
    sh.q, sh.qt = L.ptr(_chk(fp8.get("q"))), L.ptr(_chk(fp8.get("qt")))
    sh.seg_slot, sh.seg_in, sh.seg_t_ld = (L.ptr(_chk(fp8.get(k), torch.int32)) for k in ("seg_slot", "seg_in", "seg_t_ld"))
    sh.scale, sh.amax = L.ptr(_chk(fp8.get("scale"), torch.float32)), L.ptr(_chk(fp8.get("amax"), torch.float32))
    sh.seg_t_base = L.ptr(_chk(fp8.get("seg_t_base"), torch.int64))
    return sh, C.byref(sh)


def adamw_step(p, g, m, v, seg_off, seg_len, seg_lr, seg_wd, blk_seg, blk_off, step=1, betas=(0.9, 0.999), eps=1e-8, p_bf16=None,
               inv_scale=None, amp=None, fp8=None, max_workgroups=0, zero_grads=False, g_bf16=None, ema=None, ema_weight=0.0):
    """crct_adamw_step in place on the flat fp32 buffers p, g, m, v over the device tables (seg_*, blk_* from ``adamw_plan``).
    inv_scale: device fp32 scalar; amp / fp8: dicts of device tensors named after the fields of CrctAmpState / CrctFp8Shadow.
    ema (flat fp32, the element offsets of p): crct_adamw_step_ema instead -- ema += ema_weight * (p' - ema) in the same launch."""
    amp_keep, amp_arg = _amp_state(amp)
    f8_keep, f8_arg = _fp8_shadow(fp8)
    args = (L.ptr(_chk(p, torch.float32)), L.ptr(_chk(g, torch.float32)), L.ptr(_chk(m, torch.float32)),
            L.ptr(_chk(v, torch.float32)), L.ptr(_chk(p_bf16, torch.bfloat16)), L.ptr(_chk(seg_off, torch.int64)),
            L.ptr(_chk(seg_len, torch.int64)), L.ptr(_chk(seg_lr, torch.float32)), L.ptr(_chk(seg_wd, torch.float32)),
            L.ptr(_chk(blk_seg, torch.int32)), L.ptr(_chk(blk_off, torch.int64)), blk_seg.numel(),
            float(betas[0]), float(betas[1]), float(eps), int(step), L.ptr(_chk(inv_scale, torch.float32)),
            amp_arg, f8_arg, int(max_workgroups), int(bool(zero_grads)), L.ptr(_chk(g_bf16, torch.bfloat16)))
    if ema is None:
        L.check(L.load().crct_adamw_step(*args, L.current_stream()), "adamw_step")
    else:
        L.check(L.load().crct_adamw_step_ema(*args, L.ptr(_chk(ema, torch.float32)), float(ema_weight), L.current_stream()), "adamw_step_ema")


def adamw_advance(step_dev, found_inf=None):
    """crct_adamw_advance: the device step counter (int32 [1]) += 1 unless found_inf (device fp32 [1], optional) is set."""
    L.check(L.load().crct_adamw_advance(L.ptr(_chk(step_dev, torch.int32)), L.ptr(_chk(found_inf, torch.float32)), L.current_stream()),
            "adamw_advance")


def fp8_update_scales(scale, amax, n=None, reset=False, skip_if=None, fmax=448.0):
    """crct_fp8_update_scales over the first n entries (default: all of ``scale``); amax holds FP8_AMAX_LANES words per entry."""
    n = scale.numel() if n is None else int(n)
    L.check(L.load().crct_fp8_update_scales(L.ptr(_chk(scale, torch.float32)), L.ptr(_chk(amax, torch.float32)), n, int(bool(reset)),
                                            L.ptr(_chk(skip_if, torch.float32)), float(fmax), L.current_stream()), "fp8_update_scales")


def fp8_quantize_bf16(x, q, scale, amax=None):
    """crct_fp8_quantize_bf16: q (uint8, x.numel() bytes) = e4m3(x * *scale); max |x| max-ed into amax when given."""
    L.check(L.load().crct_fp8_quantize_bf16(L.ptr(_chk(x, torch.bfloat16)), L.ptr(_chk(q, torch.uint8)), L.ptr(_chk(scale, torch.float32)),
                                            L.ptr(_chk(amax, torch.float32)), x.numel(), L.current_stream()), "fp8_quantize_bf16")
    return q


def fp8_quantize_weights(p, q, seg_off, seg_len, seg_slot, blk_seg, blk_off, scale, amax):
    """crct_fp8_quantize_weights: the exact per-tensor quantisation of the segments with seg_slot >= 0 into the flat byte buffer q."""
    L.check(L.load().crct_fp8_quantize_weights(L.ptr(_chk(p, torch.float32)), L.ptr(_chk(q, torch.uint8)), L.ptr(_chk(seg_off, torch.int64)),
                                               L.ptr(_chk(seg_len, torch.int64)), L.ptr(_chk(seg_slot, torch.int32)),
                                               L.ptr(_chk(blk_seg, torch.int32)), L.ptr(_chk(blk_off, torch.int64)), blk_seg.numel(),
                                               L.ptr(_chk(scale, torch.float32)), L.ptr(_chk(amax, torch.float32)), scale.numel(),
                                               L.current_stream()), "fp8_quantize_weights")
    return q


def fp8_transpose_weights(q, qt, w_off, w_out, w_in, max_workgroups=0):
    """crct_fp8_transpose_weights of the weights (byte offset, out, in) given as host sequences; builds the tile table."""
    tiles = [((o + 63) // 64) * ((i + 63) // 64) for o, i in zip(w_out, w_in)]
    begin = [sum(tiles[:k]) for k in range(len(tiles))]
    dev = q.device
    t = (torch.tensor(list(w_off), dtype=torch.int64, device=dev), torch.tensor(list(w_out), dtype=torch.int32, device=dev),
         torch.tensor(list(w_in), dtype=torch.int32, device=dev), torch.tensor(begin, dtype=torch.int64, device=dev))
    L.check(L.load().crct_fp8_transpose_weights(L.ptr(_chk(q, torch.uint8)), L.ptr(_chk(qt, torch.uint8)), t[0].data_ptr(), t[1].data_ptr(),
                                                t[2].data_ptr(), t[3].data_ptr(), len(tiles), sum(tiles), int(max_workgroups),
                                                L.current_stream()), "fp8_transpose_weights")
    torch.cuda.current_stream().synchronize()        # the tables above must outlive the launch
    return qt


def cast_f32(x, out=None):
    """crct_cast_bf16_f32: bf16 -> fp32"""
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.load().crct_cast_bf16_f32(L.ptr(_chk(x, torch.bfloat16)), L.ptr(_chk(out, torch.float32)), x.numel(), L.current_stream()), "cast")
    return out


def cast_runs(x, y, run_off, run_len, blk_seg, blk_off):
    """y[off[r] + i] = cast(x[off[r] + i]) over the runs of an ``adamw_plan`` table: fp32 -> bf16 or bf16 -> fp32 by the dtypes."""
    lib = L.load()
    if x.dtype == torch.float32 and y.dtype == torch.bfloat16:
        fn = lib.crct_cast_runs_f32_bf16
    elif x.dtype == torch.bfloat16 and y.dtype == torch.float32:
        fn = lib.crct_cast_runs_bf16_f32
    else:
        raise TypeError("cast_runs: fp32 -> bf16 or bf16 -> fp32 (got %s -> %s)" % (x.dtype, y.dtype))
    L.check(fn(L.ptr(_chk(x)), L.ptr(_chk(y)), L.ptr(_chk(run_off, torch.int64)), L.ptr(_chk(run_len, torch.int64)),
               L.ptr(_chk(blk_seg, torch.int32)), L.ptr(_chk(blk_off, torch.int64)), blk_seg.numel(), L.current_stream()), "cast_runs")
    return y


def zero_runs(g, run_off, run_len, blk_seg, blk_off):
    """crct_zero_runs: g[off[r] .. off[r] + len[r]) = 0 over the runs of an ``adamw_plan`` table."""
    L.check(L.load().crct_zero_runs(L.ptr(_chk(g, torch.float32)), L.ptr(_chk(run_off, torch.int64)), L.ptr(_chk(run_len, torch.int64)),
                                    L.ptr(_chk(blk_seg, torch.int32)), L.ptr(_chk(blk_off, torch.int64)), blk_seg.numel(),
                                    L.current_stream()), "zero_runs")
    return g


# ---- masked-LM head (csrc/lm_head.hip): the row kernels around the three vocabulary-sized GEMMs on padded operands
def pad64(n):
    return (int(n) + 63) // 64 * 64


def lm_gather_rows(src, rows, R, Rp=None):
    """bf16 [Rp, H]: row r < R = bf16(src[rows[r]]) (src fp32 [N, H], rows int32 on the device), the pad rows +0 (crct_lm_gather_rows)."""
    H = src.shape[-1]
    Rp = pad64(max(R, 1)) if Rp is None else int(Rp)
    out = torch.empty(Rp, H, device=src.device, dtype=torch.bfloat16)
    L.check(L.load().crct_lm_gather_rows(L.ptr(_chk(src, torch.float32)), L.ptr(_chk(rows, torch.int32)), L.ptr(out), int(R), Rp, H,
                                         L.current_stream()), "lm_gather_rows")
    return out


def lm_scatter_rows(src, rows, dst, R):
    """dst[rows[r]] = src[r] for r < R (fp32, distinct rows; the rest of dst is untouched) (crct_lm_scatter_rows)."""
    H = src.shape[-1]
    L.check(L.load().crct_lm_scatter_rows(L.ptr(_chk(src, torch.float32)), L.ptr(_chk(rows, torch.int32)), L.ptr(_chk(dst, torch.float32)),
                                          int(R), H, L.current_stream()), "lm_scatter_rows")
    return dst


def lm_pad_operands(table, bias, table_pad=None, bias_pad=None):
    """(bf16 [Vp, H] copy of the bf16 table [V, H] with zero pad rows, fp32 [Vp] copy of the fp32 bias [V] with zero pad), Vp = pad64(V)."""
    V, H = table.shape
    Vp = pad64(V)
    table_pad = torch.empty(Vp, H, device=table.device, dtype=torch.bfloat16) if table_pad is None else table_pad
    bias_pad = torch.empty(Vp, device=table.device, dtype=torch.float32) if bias_pad is None else bias_pad
    L.check(L.load().crct_lm_pad_operands(L.ptr(_chk(table, torch.bfloat16)), L.ptr(_chk(bias, torch.float32)), L.ptr(table_pad), L.ptr(bias_pad),
                                          V, Vp, H, L.current_stream()), "lm_pad_operands")
    return table_pad, bias_pad


def lm_ce_fwd(logits, labels, R, V, inv_n):
    """(loss fp32 [R], lse fp32 [R], lm_loss fp32 [1, 1] = inv_n * sum loss) over the first V columns of the fp32 logits [>= R, ld]."""
    dev = logits.device
    loss, lse, total = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(1, 1, device=dev)
    L.check(L.load().crct_lm_ce_fwd(L.ptr(_chk(logits, torch.float32)), logits.stride(0), L.ptr(_chk(labels, torch.int32)), L.ptr(loss), L.ptr(lse),
                                    L.ptr(total), int(R), int(V), float(inv_n), L.current_stream()), "lm_ce_fwd")
    return loss, lse, total


def lm_ce_bwd(logits, labels, lse, g, inv_n, R, V):
    """dL bf16 [Rp, Vp] = (softmax - onehot) * g * inv_n over the real rows and columns, +0 in every pad row and column; g: device fp32 scalar."""
    Rp, Vp = logits.shape
    dL = torch.empty(Rp, Vp, device=logits.device, dtype=torch.bfloat16)
    L.check(L.load().crct_lm_ce_bwd(L.ptr(_chk(logits, torch.float32)), logits.stride(0), L.ptr(_chk(labels, torch.int32)), L.ptr(_chk(lse, torch.float32)),
                                    L.ptr(_chk(g, torch.float32)), float(inv_n), L.ptr(dL), Vp, int(R), Rp, int(V), Vp, L.current_stream()), "lm_ce_bwd")
    return dL


def lm_add(dst, src, n, accumulate=True):
    """dst.flatten()[:n] (+)= src.flatten()[:n] (fp32, contiguous); nothing at or past n is touched (crct_lm_add_f32)."""
    L.check(L.load().crct_lm_add_f32(L.ptr(_chk(dst, torch.float32)), L.ptr(_chk(src, torch.float32)), int(n), int(bool(accumulate)),
                                     L.current_stream()), "lm_add")
    return dst


def lm_gelu_bwd(dy, pre):
    """bf16(dy * gelu'(pre)), bf16 tensors of one shape (crct_lm_gelu_bwd)."""
    dx = torch.empty_like(dy)
    L.check(L.load().crct_lm_gelu_bwd(L.ptr(_chk(dy, torch.bfloat16)), L.ptr(_chk(pre, torch.bfloat16)), L.ptr(dx), dy.numel(), L.current_stream()),
            "lm_gelu_bwd")
    return dx


def lm_decoder_wgrad(dL, z, out, V, accumulate=True):
    """out fp32 [V, H] (+)= (dL^T z)[:V]: the decoder's weight gradient onto the word-table gradient.  dL bf16 [Rp, Vp], z bf16 [Rp, H].  The
    transposed operand's extent must be a multiple of 8 and V is not, so the product goes to an own fp32 [Vp, H] scratch and its first V rows
    are added (or written) by a row kernel: whatever follows ``out`` in memory is never touched."""
    Rp, Vp = dL.shape
    H = z.shape[1]
    scratch = gemm(dL, z, Vp, H, Rp, ta=True, tb=True, out_f32=True)
    return lm_add(out, scratch, V * H, accumulate)


def lm_topk_rows(logits, R, V, k, labels=None):
    """The k first columns of each of the first R rows of the fp32 logits [>= R, ld] over their first V columns, in the order "larger value
    first, then smaller column" (NaN above +inf, -0 below +0): (ids int32 [R, k], logprob fp32 [R, k] = x - lse, lse fp32 [R], label_logprob
    fp32 [R], label_rank int32 [R]); the last two are None without ``labels`` (int32 [R] on the device).  ``label_rank`` counts the columns in
    front of the label, so ``rank < k`` is "label in the top k"; ``lse`` holds the bits of ``lm_ce_fwd``'s.  k in {1, 5, 8}, V >= k and a row
    stride that is a multiple of 4 -- anything else is refused before a launch; R == 0 launches nothing (crct_lm_topk_rows)."""
    dev = logits.device
    R, k = int(R), int(k)
    ids, logprob = torch.empty(R, k, dtype=torch.int32, device=dev), torch.empty(R, k, device=dev)
    lse = torch.empty(R, device=dev)
    lab_lp = torch.empty(R, device=dev) if labels is not None else None
    lab_rank = torch.empty(R, dtype=torch.int32, device=dev) if labels is not None else None
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < R:
        raise ValueError("lm_topk_rows: logits must be [>= R, ld] with unit column stride")
    L.check(L.load().crct_lm_topk_rows(L.ptr(_chk(logits, torch.float32)), logits.stride(0), L.ptr(_chk(labels, torch.int32)), L.ptr(ids), L.ptr(logprob),
                                       L.ptr(lse), L.ptr(lab_lp), L.ptr(lab_rank), R, int(V), k, L.current_stream()), "lm_topk_rows")
    return ids, logprob, lse, lab_lp, lab_rank


def lm_scores_grad_pack(g, R, Rp, V, Vp, c, out=None):
    """dL bf16 [Rp, Vp] = bf16(c * g[:R, :V]) with every pad row and pad column +0, from fp32 g [>= R, ldg] (unit column stride, a row stride
    that is a multiple of 4): an upstream gradient on the logits in the form ``lm_ce_bwd`` leaves the loss's (crct_lm_scores_grad_pack)."""
    if g.dim() != 2 or g.stride(1) != 1 or g.shape[0] < R:
        raise ValueError("lm_scores_grad_pack: g must be [>= R, ldg] with unit column stride")
    dL = torch.empty(int(Rp), int(Vp), device=g.device, dtype=torch.bfloat16) if out is None else out
    L.check(L.load().crct_lm_scores_grad_pack(L.ptr(_chk(g, torch.float32)), g.stride(0), float(c), L.ptr(_chk(dL, torch.bfloat16)), dL.stride(0), int(R), int(Rp),
                                              int(V), int(Vp), L.current_stream()), "lm_scores_grad_pack")
    return dL


# ---- masked-region head (csrc/region_head.hip): the two loss kernels; the rest of the head is the lm_* machinery above
def _region_targets(labels, targets, rows, C):
    if (labels is None) == (targets is None):
        raise ValueError("region_ce: give either labels (hard) or targets with rows (soft)")
    if targets is not None:
        if rows is None or targets.dim() != 2 or targets.shape[1] != C or not targets.is_contiguous():
            raise ValueError("region_ce: soft targets are a contiguous fp32 [N, C = %d] tensor read at rows (int32 [R])" % C)
    return _chk(labels, torch.int32), _chk(targets, torch.float32), _chk(rows, torch.int32) if targets is not None else None


def region_ce_fwd(logits, R, C, inv_n, labels=None, targets=None, rows=None):
    """(loss fp32 [R], lse fp32 [R], img_loss fp32 [1, 1] = inv_n * sum loss) over the first C columns of the fp32 logits [>= R, ld].  Hard:
    ``labels`` int32 [R]; soft: ``targets`` fp32 [N, C] read in place at ``rows`` int32 [R] (crct_region_ce_fwd)."""
    dev = logits.device
    labels, targets, rows = _region_targets(labels, targets, rows, int(C))
    loss, lse, total = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(1, 1, device=dev)
    L.check(L.load().crct_region_ce_fwd(L.ptr(_chk(logits, torch.float32)), logits.stride(0), L.ptr(labels), L.ptr(targets), L.ptr(rows), L.ptr(loss),
                                        L.ptr(lse), L.ptr(total), int(R), int(C), float(inv_n), L.current_stream()), "region_ce_fwd")
    return loss, lse, total


def region_ce_bwd(logits, lse, g, inv_n, R, C, labels=None, targets=None, rows=None):
    """dL bf16 [Rp, Cp] = (softmax * s_r - t) * g * inv_n over the real rows and columns (s_r = sum_j t_rj; hard: t the one-hot), +0 in every
    pad row and column; g: device fp32 scalar (crct_region_ce_bwd)."""
    Rp, Cp = logits.shape
    labels, targets, rows = _region_targets(labels, targets, rows, int(C))
    dL = torch.empty(Rp, Cp, device=logits.device, dtype=torch.bfloat16)
    L.check(L.load().crct_region_ce_bwd(L.ptr(_chk(logits, torch.float32)), logits.stride(0), L.ptr(labels), L.ptr(targets), L.ptr(rows),
                                        L.ptr(_chk(lse, torch.float32)), L.ptr(_chk(g, torch.float32)), float(inv_n), L.ptr(dL), Cp, int(R), Rp, int(C), Cp,
                                        L.current_stream()), "region_ce_bwd")
    return dL
