"""Poisoned operands through the kernels (-m gpu): the NaN / inf footprint of every kernel family against the fp64 references
("Non-finite values"; tests/poison_ref.py states R1 - R3).

Every case makes two launches on the same buffers, clean and with one or two non-finite input elements.  The reference, run on the
poisoned inputs on the CPU, names the outputs that must turn non-finite (R1); every other output element keeps the bits of the
clean launch (R2).  R4, the ignored memory: every operand lies in a buffer whose stride padding and whose rows behind the last row
(at least one tile of them) hold NaN, every output lies in a canvas of NaN, and the CLEAN launch must still give the exact (or the
unpoisoned kernel's) result -- a kernel that reads a column past K, a row past M or a key past Tk as data cannot.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import gemm_ref as GR            # noqa: E402
import attention_ref as AR       # noqa: E402
import poison_ref as PR          # noqa: E402
from poison_ref import NAN, INF  # noqa: E402
from test_kernels_gpu import (GEMM_CFGS, DROP_SEEDS, _assert_bits, _assert_sums, _assert_within_bf16_step, _check_ln_forward,   # noqa: E402
                              _check_ln_forward_terms, _f8, _ln_backward64, _ln_check_backward, _ln_stats64, _logged, _ran_cfg, bf,
                              host_keep, rand)
import input_grad_ref as IG      # noqa: E402
from test_attention_gpu import _hooks   # noqa: E402

DEV = "cuda"
PAD = 128                      # NaN rows behind every operand: one tile of the largest configuration


@pytest.fixture(params=["pipelined", "generic"])
def gemm_path(request):
    """As tests/test_kernels_gpu.py's, for the GEMM tests only: the LDS-DMA kernels, and every GEMM forced through the register-staged one."""
    lib = L.load()
    lib.crct_gemm_force_generic(int(request.param == "generic"))
    yield request.param
    lib.crct_gemm_force_generic(0)


# ------------------------------------------------------------------------------------------- buffers of ignored memory
def _nan_rows(x, ld=None, pad=PAD):
    """x [r][c] (fp64, CPU) in the first c columns of a [r + pad][ld] buffer of NaN, on the GPU."""
    return GR.strided(x, ld or x.shape[1], rows=x.shape[0] + pad, fill=NAN).to(DEV)


class _Canvas:
    """[M + 3][ld] output buffer of NaN (or [M][N] = inner); after the launches every element outside [M][N] must still be NaN."""

    def __init__(self, M, N, ld, dtype, inner=None):
        self.M, self.N = M, N
        self.buf = torch.full((M + 3, ld), NAN, device=DEV, dtype=dtype)
        if inner is not None:
            self.buf[:M, :N] = inner.to(dtype)

    @property
    def out(self):
        return self.buf[:self.M, :self.N]

    def intact(self, what):
        mask = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        mask[:self.M, :self.N] = False
        bad = mask & ~torch.isnan(self.buf)
        assert not bool(bad.any()), "%s: %d elements outside [%d, %d] of the output buffer were written, first at %s" % (
            what, int(bad.sum()), self.M, self.N, tuple(int(i) for i in bad.nonzero()[0]))
        return self.out


def _lay(a, b, layout):
    """a [M][K], b [N][K] (fp64, CPU) -> the bf16 operands of a launch in `layout` with their leading dimensions: stride padding and
    PAD rows behind each operand are NaN."""
    (M, K), N = a.shape, b.shape[0]
    if layout == "nt":
        A, B, kw = _nan_rows(a, K + 16), _nan_rows(b, K + 8), dict(lda=K + 16, ldb=K + 8)
    elif layout == "tb":
        A, B, kw = _nan_rows(a, K + 16), _nan_rows(b.t(), N + 8), dict(tb=True, lda=K + 16, ldb=N + 8)
    else:
        A, B, kw = _nan_rows(a.t(), M + 8), _nan_rows(b.t(), N + 8), dict(ta=True, tb=True, lda=M + 8, ldb=N + 8)
    return bf(A), bf(B), kw


def _gemm(a, b, layout, out_f32=False, ldc_extra=24, prev=None, expect=None, **kw):
    """One launch of a [M][K] x b [N][K] in `layout` from NaN-padded operands into a NaN canvas; returns the output [M][N]."""
    (M, K), N = a.shape, b.shape[0]
    A, B, lkw = _lay(a, b, layout)
    cv = _Canvas(M, N, N + ldc_extra, torch.float32 if out_f32 else torch.bfloat16, inner=prev)
    _, recs = _logged(lambda: ops.gemm(A, B, M, N, K, out=cv.buf, ldc=N + ldc_extra, **lkw, **kw))
    if expect is not None:
        assert recs == [expect], (recs, expect)
    return cv.intact("gemm %s %dx%dx%d" % (layout, M, N, K)).clone()


def _poison_sites(M, K):
    """A's NaN: the last element, the first, and one on a tile boundary of every configuration (row 128; k = 64 where K has it)."""
    return ((M - 1, K - 1), (0, 0), (128, 64 if K > 64 else K - 1))


def _gemm_footprints(run, a, b, ref_fn, what, exact=True):
    """run(a, b) -> output [M][N].  Clean launch (exact against ref_fn when `exact`), then one launch per NaN site of A, each with an inf
    in B at (n = 129, k = 0) (n = N - 1 for a narrower B): F = that row united with that column."""
    (M, K), N = a.shape, b.shape[0]
    clean = run(a, b)
    if exact:
        _assert_bits(clean, ref_fn(a, b), what + ": clean launch from NaN-padded buffers")
    for (m, k) in _poison_sites(M, K):
        if m >= M:
            continue
        n = 129 if N > 129 else N - 1
        ap, bp = PR.plant(a, (m, k), NAN), PR.plant(b, (n, 0), INF)
        F = PR.footprint(ref_fn, (a, b), (ap, bp))
        want = torch.zeros(M, N, dtype=torch.bool)
        want[m, :] = True
        want[:, n] = True
        assert torch.equal(F, want), what                     # the closed form, once more
        PR.assert_footprint(clean, run(ap, bp), F, "%s, NaN at A(%d, %d), inf at B(%d, 0)" % (what, m, k, n))


# ------------------------------------------------------------------------------------------- bf16 GEMM
@pytest.mark.parametrize("layout", ["nt", "tb", "tt"])
@pytest.mark.parametrize("tile", GEMM_CFGS)
def test_gemm_footprint_every_configuration_and_layout(tile, layout, gemm_path):
    M, N = (264 if layout == "tt" else 257), 200
    for K in (64, 192):
        a, b = GR.operands(M, N, K, 48, 48, seed=K + tile, ea=-3, eb=-5)
        expect = (_ran_cfg(gemm_path, tile, M, N, K), 1, 1)
        for out_f32 in (False, True):
            rnd = GR.f32 if out_f32 else GR.bf16
            _gemm_footprints(lambda x, y: _gemm(x, y, layout, out_f32=out_f32, tile=tile, expect=expect), a, b,
                             lambda x, y: rnd(GR.ref_nt(x, y)), "cfg %d %s K=%d %s" % (tile, layout, K, "fp32" if out_f32 else "bf16"))


@pytest.mark.parametrize("layout,M,N,K,t", [("nt", 77, 12, 72, 3), ("tb", 97, 104, 776, 3)])
def test_gemm_footprint_register_staged_kernel(layout, M, N, K, t, gemm_path):
    a, b = GR.operands(M, N, K, 64, 64, seed=M + N + K, ea=-3, eb=-5)
    _gemm_footprints(lambda x, y: _gemm(x, y, layout, expect=(16 + t, 1, 1)), a, b, lambda x, y: GR.bf16(GR.ref_nt(x, y)),
                     "register-staged %s %dx%dx%d" % (layout, M, N, K))


@pytest.mark.parametrize("tile", (4, 9))
def test_gemm_footprint_split_k(tile, gemm_path):
    """S = 3 over K = 768: the slabs of the three slices are summed by the last workgroup of a tile -- a NaN in one slice's slab
    reaches exactly the rows / columns of its operand element."""
    M, N, K, S = 257, 200, 768, 3
    split = S if gemm_path == "pipelined" else 1
    for layout in ("nt", "tb"):
        a, b = GR.operands(M, N, K, 48, 48, seed=tile + len(layout), ea=-3, eb=-5)
        expect = (_ran_cfg(gemm_path, tile, M, N, K), split, 1)
        _gemm_footprints(lambda x, y: _gemm(x, y, layout, out_f32=True, tile=tile, split_k=S, expect=expect), a, b,
                         lambda x, y: GR.f32(GR.ref_nt(x, y)), "split-K cfg %d %s" % (tile, layout))


def test_gemm_footprint_grouped_forward_pair(gemm_path):
    """Two problems in ONE grid: the poison sits in problem 1, problem 0 keeps its bits."""
    shapes = [(257, 200, 192), (130, 264, 64)]
    ab = [GR.operands(M, N, K, 24, 24, seed=3 + i, ea=-3, eb=-5) for i, (M, N, K) in enumerate(shapes)]

    def run(pairs):
        probs, cvs = [], []
        for (a, b), (M, N, K) in zip(pairs, shapes):
            A, B, kw = _lay(a, b, "nt")
            cvs.append(_Canvas(M, N, N + 24, torch.bfloat16))
            probs.append(dict(A=A, B=B, M=M, N=N, K=K, out=cvs[-1].buf, ldc=N + 24, tile=9, **kw))
        _, recs = _logged(lambda: ops.gemm_grouped(probs))
        assert recs == ([(9, 1, 2)] if gemm_path == "pipelined" else [(_ran_cfg(gemm_path, 9, *s), 1, 1) for s in shapes]), recs
        return [cv.intact("grouped pair").clone() for cv in cvs]

    def ref(a0, b0, a1, b1):
        return GR.bf16(GR.ref_nt(a0, b0)), GR.bf16(GR.ref_nt(a1, b1))
    clean = run(ab)
    for got, (a, b) in zip(clean, ab):
        _assert_bits(got, GR.bf16(GR.ref_nt(a, b)), "grouped pair: clean")
    pois = [ab[0], (PR.plant(ab[1][0], (129, 63), NAN), PR.plant(ab[1][1], (0, 0), INF))]
    F = PR.footprint(ref, (*ab[0], *ab[1]), (*pois[0], *pois[1]))
    assert int(F[0].sum()) == 0 and int(F[1].sum()) == 264 + 130 - 1
    PR.assert_footprint(clean, run(pois), F, "grouped forward pair")


def test_gemm_footprint_grouped_weight_gradients(gemm_path):
    """Eight weight gradients dW += dy^T x of one launch, R = 129 tokens, the token rows behind R are NaN.  In problem 5, dy's NaN
    element (r, n) reaches row n of that dW and x's inf element (r, k) its column k; the other seven problems keep their bits."""
    R = 129
    shapes = [(144, 208), (64, 64), (200, 136), (136, 264), (72, 520), (264, 72), (128, 192), (16, 48)]
    data = [(GR.ints((R, N), 32, 50 + i) / 8, GR.ints((R, K), 32, 60 + i) / 32, GR.unit_ints((N, K), 64, 70 + i, 2.0 ** -8))
            for i, (N, K) in enumerate(shapes)]

    def run(items):
        probs = []
        for dy, x, pre in items:
            probs.append((bf(_nan_rows(dy))[:R], bf(_nan_rows(x))[:R], pre.float().to(DEV)))
        ops.gemm_wgrad_grouped(probs)
        return [p[2] for p in probs]

    def ref(*flat):
        return tuple(GR.f32(GR.ref_tt(flat[3 * i], flat[3 * i + 1]) + flat[3 * i + 2]) for i in range(len(shapes)))
    clean = run(data)
    for i, (got, want) in enumerate(zip(clean, ref(*[t for d in data for t in d]))):
        _assert_bits(got, want, "grouped weight gradient %d: clean" % i)
    pois = list(data)
    pois[5] = (PR.plant(data[5][0], (R - 1, 263), NAN), PR.plant(data[5][1], (0, 0), INF), data[5][2])
    F = PR.footprint(ref, [t for d in data for t in d], [t for d in pois for t in d])
    assert [int(f.sum()) for f in F] == [0, 0, 0, 0, 0, 72 + 264 - 1, 0, 0]
    PR.assert_footprint(clean, run(pois), F, "grouped weight gradients")


# ------------------------------------------------------------------------------------------- GEMM epilogues
_EPI_CASES = [("nt", 130, 100, 72, -1), ("nt", 333, 264, 192, 15)]


def _epi_inputs(M, N, K, seed):
    unit = 2.0 ** -12
    a, b = GR.operands(M, N, K, 16, 16, seed, ea=-6, eb=-6, extra=1 << 16)
    return dict(a=a, b=b, bias=GR.unit_ints((N,), 255, 1, unit * 4), add_b=GR.unit_ints((M, N), 255, 2, unit * 8),
                add_f=GR.unit_ints((M, N), 255, 3, unit) * 33, pre_b=GR.unit_ints((M, N), 255, 4, unit * 16),
                pre_f=GR.unit_ints((M, N), 255, 5, unit) * 77, src=GR.bf16(rand(M, N, scale=1.5, seed=13).cpu().double()))


@pytest.mark.parametrize("layout,M,N,K,tile", _EPI_CASES)
def test_gemm_footprint_of_every_side_operand(layout, M, N, K, tile, gemm_path):
    """One NaN at a time in the bias, the bf16 / fp32 addend, dact_src (gelu: the row-column element; relu and leaky: a select on
    s > 0, the NaN does NOT propagate and the launch equals the one with dact_src = -1 there) and the prefilled output under accumulate.
    The side operands lie in NaN-padded buffers of their own leading dimension."""
    inp = _epi_inputs(M, N, K, seed=M + K)
    a, b = inp["a"], inp["b"]
    m, n = M - 1, N - 3
    keep = host_keep(DROP_SEEDS[0], 16, M, N, 0.5).cpu()
    drop = dict(p_drop=0.5, site=16, seed=DROP_SEEDS[0])

    def side(x, dtype, ld):
        return _nan_rows(x, ld).to(dtype)

    # bias: column n of a bias -> relu -> dropout -> bf16 addend chain (dropped elements of the column are 0)
    def run_bias(bias, add):
        return _gemm(a, b, layout, tile=tile, bias=_nan_rows(bias[None, :], N + 8, pad=0)[0].float().contiguous(), act="relu",
                     addend=side(add, torch.bfloat16, N + 16), ld_add=N + 16, **drop)

    def ref_bias(bias, add):
        return GR.epilogue(GR.ref_nt(a, b), bias=bias, act="relu", keep=keep, drop_scale=2.0, addend=add)["y"]
    clean = run_bias(inp["bias"], inp["add_b"])
    _assert_bits(clean, ref_bias(inp["bias"], inp["add_b"]), "bias chain: clean")
    pb = PR.plant(inp["bias"], n, NAN)
    F = PR.footprint(ref_bias, (inp["bias"], inp["add_b"]), (pb, inp["add_b"]))
    assert 0 < int(F.sum()) < M and not bool(F[:, :n].any())
    PR.assert_footprint(clean, run_bias(pb, inp["add_b"]), F, "NaN bias")
    pa = PR.plant(inp["add_b"], (m, n), INF)
    F = PR.footprint(ref_bias, (inp["bias"], inp["add_b"]), (inp["bias"], pa))
    assert int(F.sum()) == 1
    PR.assert_footprint(clean, run_bias(inp["bias"], pa), F, "inf bf16 addend")

    # fp32 addend into an fp32 c_cached output
    def run_f(add):
        return _gemm(a, b, layout, out_f32=True, ldc_extra=8, tile=tile, addend=side(add, torch.float32, N + 8), ld_add=N + 8, c_cached=True)

    def ref_f(add):
        return GR.epilogue(GR.ref_nt(a, b), addend=add, out="f32")["y"]
    clean = run_f(inp["add_f"])
    _assert_bits(clean, ref_f(inp["add_f"]), "fp32 addend: clean")
    pa = PR.plant(inp["add_f"], (0, 0), NAN)
    PR.assert_footprint(clean, run_f(pa), PR.footprint(ref_f, (inp["add_f"],), (pa,)), "NaN fp32 addend")

    # dact_src
    for dact in ("gelu", "relu", "leaky"):
        def run_d(src):
            return _gemm(a, b, layout, tile=tile, dact_src=side(src, torch.bfloat16, N + 16), ld_aux=N + 16, dact=dact)

        def ref_d(src):
            return GR.epilogue(GR.ref_nt(a, b), dact=dact, dact_src=src)["y"]
        clean = run_d(inp["src"])
        ps = PR.plant(inp["src"], (m, n), NAN)
        got = run_d(ps)
        if dact == "gelu":
            PR.assert_footprint(clean, got, PR.footprint(ref_d, (inp["src"],), (ps,)), "NaN dact_src (gelu)")
        else:
            assert not bool(PR.nonfinite(ref_d(ps)).any())
            _assert_bits(got, run_d(PR.plant(inp["src"], (m, n), -1.0)), "NaN dact_src (%s) selects the s <= 0 branch" % dact)
            if dact == "relu":         # an exact 0 / 1 factor
                _assert_bits(got, ref_d(ps), "NaN dact_src (relu) against the reference")

    # the prefilled output under accumulate (bf16 and fp32)
    for out_f32, pre in ((False, inp["pre_b"]), (True, inp["pre_f"])):
        def run_p(prev):
            return _gemm(a, b, layout, out_f32=out_f32, tile=tile, accumulate=True, prev=prev)

        def ref_p(prev):
            return GR.epilogue(GR.ref_nt(a, b), prev=prev, out="f32" if out_f32 else "bf16")["y"]
        clean = run_p(pre)
        _assert_bits(clean, ref_p(pre), "accumulate: clean")
        pp = PR.plant(pre, (m, 0), -INF)
        PR.assert_footprint(clean, run_p(pp), PR.footprint(ref_p, (pre,), (pp,)), "-inf prefilled output, fp32 %d" % out_f32)


@pytest.mark.parametrize("act", ["relu", "gelu", "leaky", "tanh"])
@pytest.mark.parametrize("layout,M,N,K,tile", _EPI_CASES)
def test_gemm_footprint_through_an_activation(layout, M, N, K, tile, act, gemm_path):
    """A NaN element of A under bias -> preact_out -> act -> dropout at p = 0.5: its row of preact_out, and the KEPT elements of its row
    of y (a dropped NaN is 0).  relu must keep the NaN: x > 0 ? x : 0 prints 0."""
    inp = _epi_inputs(M, N, K, seed=M + K + 1)
    b, bias = inp["b"], inp["bias"]
    keep = host_keep(DROP_SEEDS[1], 41, M, N, 0.5).cpu()
    m = 128 if M > 128 else M - 1

    def run(a):
        A, B, kw = _lay(a, b, layout)
        y, pre = _Canvas(M, N, N + 24, torch.bfloat16), _Canvas(M, N, N + 16, torch.bfloat16)
        ops.gemm(A, B, M, N, K, out=y.buf, ldc=N + 24, bias=bias.float().to(DEV), act=act, preact_out=pre.buf, ld_aux=N + 16, p_drop=0.5,
                 site=41, seed=DROP_SEEDS[1], tile=tile, **kw)
        return dict(y=y.intact(act + ": y").clone(), pre=pre.intact(act + ": preact_out").clone())

    def ref(a):
        r = GR.epilogue(GR.ref_nt(a, b), bias=bias, act=act, keep=keep, drop_scale=2.0)
        return dict(y=r["y"], pre=r["pre"])
    clean = run(inp["a"])
    _assert_bits(clean["pre"], ref(inp["a"])["pre"], act + ": preact_out, clean")
    if act == "relu":
        _assert_bits(clean["y"], ref(inp["a"])["y"], "relu: clean")
    ap = PR.plant(inp["a"], (m, K - 1), NAN)
    F = PR.footprint(ref, (inp["a"],), (ap,))
    assert torch.equal(F["y"][m], keep[m]) and int(F["y"].sum()) == int(keep[m].sum()) and int(F["pre"].sum()) == N
    PR.assert_footprint(clean, run(ap), F, "NaN through %s" % act)


def test_gemm_footprint_rowsum_out(gemm_path):
    """rowsum_out (the bias gradient of a weight-gradient launch): dy's NaN element (r, m) reaches word m only."""
    M, N, R = 136, 200, 192
    at, bt = GR.ints((R, M), 32, 1) / 8, GR.ints((R, N), 32, 2) / 32
    if gemm_path == "generic":      # the register-staged kernel has no row sums: a request is refused, nothing is computed
        with pytest.raises(RuntimeError, match="gemm"):
            ops.gemm(bf(at.to(DEV)), bf(bt.to(DEV)), M, N, R, ta=True, tb=True, out=torch.zeros(M, N, device=DEV), accumulate=True,
                     rowsum_out=torch.zeros(M, device=DEV))
        return
    pre, rs_pre = GR.unit_ints((M, N), 64, 3, 2.0 ** -8), GR.unit_ints((M,), 64, 4, 2.0 ** -3)

    def run(at):
        out = _Canvas(M, N, N + 8, torch.float32, inner=pre)
        rs = torch.full((M + 8,), NAN, device=DEV)
        rs[:M] = rs_pre.float()
        ops.gemm(bf(_nan_rows(at, M + 8)), bf(_nan_rows(bt, N + 8)), M, N, R, ta=True, tb=True, lda=M + 8, ldb=N + 8, out=out.buf,
                 ldc=N + 8, accumulate=True, rowsum_out=rs, tile=9)
        assert bool(torch.isnan(rs[M:]).all()), "rowsum_out written past M"
        return dict(dw=out.intact("rowsum: dW").clone(), rs=rs[:M].clone())

    def ref(at):
        return dict(dw=GR.f32(GR.ref_tt(at, bt) + pre), rs=GR.f32(rs_pre + at.sum(0)))
    clean = run(at)
    for k, v in ref(at).items():
        _assert_bits(clean[k], v, "rowsum clean: " + k)
    ap = PR.plant(at, (R - 1, 7), NAN)
    PR.assert_footprint(clean, run(ap), PR.footprint(ref, (at,), (ap,)), "NaN dy under rowsum_out")


def test_gemm_footprint_layernorm_addend(gemm_path):
    """crct_gemm_bf16_ln_addend: the addend is the LayerNorm of fp32 source rows, rebuilt from (mean, rstd, gamma, beta).  A NaN in
    mean[m] or rstd[m] poisons row m, one in the source its element, one in gamma its column."""
    M, N, K = 130, 104, 64
    a, b = GR.operands(M, N, K, 16, 16, 9, ea=-6, eb=-6, extra=1 << 16)
    src = rand(M, N, scale=2.0, seed=5).cpu().double()
    gamma, beta = (1 + 0.1 * rand(N, seed=6)).cpu().double(), (0.1 * rand(N, seed=7)).cpu().double()
    mean, _, rstd = _ln_stats64(GR.f32(src))
    mean, rstd = GR.f32(mean), GR.f32(rstd)

    def run(src, mean, rstd, gamma):
        ln = tuple(torch.cat([t.float(), torch.full((PAD,), NAN)]).to(DEV)[:len(t)] for t in (mean, rstd, gamma, beta))
        return _gemm(a, b, "nt", out_f32=True, ldc_extra=8, tile=9, addend=_nan_rows(src, N + 8).float(), ld_add=N + 8, c_cached=True,
                     ln_addend=ln)

    def ref(src, mean, rstd, gamma):
        return GR.f32(GR.ref_nt(a, b) + GR.f32(gamma * ((GR.f32(src) - mean[:, None]) * rstd[:, None]) + beta))
    clean_in = (src, mean, rstd, gamma)
    clean = run(*clean_in)
    # the clean launch: four fp32 roundings (x - mean, * rstd, the fused multiply-add, + acc), each 2^-24 of a term's magnitude
    terms = GR.ref_nt(a, b).abs() + (gamma * ((GR.f32(src) - mean[:, None]) * rstd[:, None])).abs() + beta.abs()
    assert bool(((clean.double().cpu() - ref(*clean_in)).abs() <= 2.0 ** -22 * terms).all()), "LayerNorm addend: clean launch"
    for i, idx, count in ((0, (M - 1, N - 1), 1), (1, M - 1, N), (2, 0, N), (3, N - 1, M)):
        pois = list(clean_in)
        pois[i] = PR.plant(clean_in[i], idx, NAN)
        F = PR.footprint(ref, clean_in, pois)
        assert int(F.sum()) == count
        PR.assert_footprint(clean, run(*pois), F, "LayerNorm addend, NaN in input %d" % i)


def test_gemm_footprint_layernorm_addend_grouped(gemm_path):
    """crct_gemm_bf16_grouped_ln_addend: two problems in one launch, each with its own LayerNorm addend.  A NaN in problem 1's mean /
    rstd row or source row poisons that row (element) of problem 1; problem 0 keeps its bits."""
    shapes = [(130, 104, 64), (77, 136, 128)]
    data = []
    for i, (M, N, K) in enumerate(shapes):
        a, b = GR.operands(M, N, K, 16, 16, 20 + i, ea=-6, eb=-6, extra=1 << 16)
        src = GR.f32(rand(M, N, scale=2.0, seed=30 + i).cpu().double())
        gamma, beta = (1 + 0.1 * rand(N, seed=40 + i)).cpu().double(), (0.1 * rand(N, seed=50 + i)).cpu().double()
        mean, _, rstd = _ln_stats64(src)
        data.append(dict(a=a, b=b, src=src, mean=GR.f32(mean), rstd=GR.f32(rstd), gamma=gamma, beta=beta))

    def run(items):
        probs, cvs = [], []
        for d, (M, N, K) in zip(items, shapes):
            A, B, kw = _lay(d["a"], d["b"], "nt")
            ln = tuple(torch.cat([d[k].float(), torch.full((PAD,), NAN)]).to(DEV)[:len(d[k])] for k in ("mean", "rstd", "gamma", "beta"))
            cvs.append(_Canvas(M, N, N + 8, torch.float32))
            probs.append(dict(A=A, B=B, M=M, N=N, K=K, out=cvs[-1].buf, ldc=N + 8, addend=_nan_rows(d["src"], N + 8).float(), ld_add=N + 8,
                              c_cached=True, ln_addend=ln, tile=9, **kw))
        ops.gemm_grouped(probs)
        return [cv.intact("grouped LayerNorm addend").clone() for cv in cvs]

    def ref(*flat):                 # (src, mean, rstd) per problem
        out = []
        for i, d in enumerate(data):
            src, mean, rstd = flat[3 * i:3 * i + 3]
            out.append(GR.f32(GR.ref_nt(d["a"], d["b"]) + GR.f32(d["gamma"] * ((src - mean[:, None]) * rstd[:, None]) + d["beta"])))
        return tuple(out)
    flat0 = [data[i][k] for i in range(2) for k in ("src", "mean", "rstd")]
    clean = run(data)
    for got, want, d in zip(clean, ref(*flat0), data):
        terms = GR.ref_nt(d["a"], d["b"]).abs() + (d["gamma"] * ((d["src"] - d["mean"][:, None]) * d["rstd"][:, None])).abs() + d["beta"].abs()
        assert bool(((got.double().cpu() - want).abs() <= 2.0 ** -22 * terms).all()), "grouped LayerNorm addend: clean launch"
    M1, N1 = shapes[1][:2]
    for key, idx, count in (("src", (M1 - 1, 0), 1), ("mean", M1 - 1, N1), ("rstd", 0, N1)):
        items = [data[0], dict(data[1], **{key: PR.plant(data[1][key], idx, NAN)})]
        F = PR.footprint(ref, flat0, [items[i][k] for i in range(2) for k in ("src", "mean", "rstd")])
        assert [int(f.sum()) for f in F] == [0, count]
        PR.assert_footprint(clean, run(items), F, "grouped LayerNorm addend, NaN in %s of problem 1" % key)


# ------------------------------------------------------------------------------------------- fp8 GEMMs
def _fp8_words():
    return torch.tensor([0.25], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)


def _assert_scale_kept_and_words_cleared(scale, amax, what):
    """crct_fp8_update_scales' rule for a non-finite maximum, here reached from a tensor: the scale stays, the words are cleared."""
    assert bool(torch.isnan(amax).any()), what + ": the NaN did not reach the amax words"
    before = scale.clone()
    ops.fp8_update_scales(scale, amax, n=1)
    assert torch.equal(scale, before) and bool(torch.isfinite(scale).all()) and float(scale) != 0.0, what + ": scale changed"
    assert float(amax.abs().max()) == 0.0, what + ": amax words not cleared"


@pytest.mark.parametrize("M,N,K,cfg", [(257, 520, 384, 20), (300, 1000, 2048, 21)])
def test_gemm_fp8_forward_footprint_and_copy(M, N, K, cfg):
    """Forward ids 20 / 21: the e4m3 NaN byte (0x7F) in A poisons its row of y, preact_out and q_out (bytes that decode to NaN), and
    q_amax holds NaN; a NaN bias element does the same to its column."""
    amax = 16 if K <= 2048 else 8
    qa, qb = GR.operands(M, N, K, amax, amax, seed=M + K, kind="e4m3", extra=1 << 16)
    bias = GR.unit_ints((N,), 255, 5, 1.0 / 32)
    sa_d, sb_d = torch.tensor([8.0], device=DEV), torch.tensor([4.0], device=DEV)

    def run(qa, bias):
        pre = torch.full((M, N), NAN, device=DEV, dtype=torch.bfloat16)
        q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
        qs, am = _fp8_words()
        nan_rows = torch.full((PAD, K), 0x7F, device=DEV, dtype=torch.uint8)          # the e4m3 NaN byte behind both operands
        xa = torch.cat([_f8(qa, "e4m3").view(torch.uint8), nan_rows])[:M]
        xb = torch.cat([_f8(qb, "e4m3").view(torch.uint8), nan_rows])[:N]
        y, recs = _logged(lambda: ops.gemm_fp8(xa, xb, sa_d, sb_d, M, N, K, bias=bias.float().to(DEV), act="relu", preact_out=pre,
                                               q_out=q_out, q_scale=qs, q_amax=am))
        assert recs == [(cfg, 1, 1)], recs
        return dict(y=y, pre=pre, q=q_out.view(torch.float8_e4m3fn)), qs, am

    def ref(qa, bias):
        r = GR.epilogue(GR.ref_nt(qa, qb), alpha=1.0 / 32, bias=bias, act="relu", q_scale=0.25, q_kind="e4m3")
        return dict(y=r["y"], pre=r["pre"], q=r["q"])
    clean, _, am = run(qa, bias)
    for k, v in ref(qa, bias).items():
        _assert_bits(PR.as_float(clean[k]), v, "fp8 forward clean: " + k)
    assert bool(torch.isfinite(am).all())
    for what, pois in (("0x7F in A", (PR.plant(qa, (M - 1, K - 1), NAN), bias)), ("NaN bias", (qa, PR.plant(bias, 129, NAN)))):
        assert what != "0x7F in A" or int(_f8(pois[0], "e4m3").view(torch.uint8)[M - 1, K - 1]) == 0x7F
        got, qs, am = run(*pois)
        F = PR.footprint(ref, (qa, bias), pois)
        PR.assert_footprint(clean, got, F, "fp8 forward, " + what)
        nan_bytes = (got["q"].view(torch.uint8) & 0x7F) == 0x7F
        assert torch.equal(nan_bytes.cpu(), F["q"]), what + ": q_out holds the NaN byte exactly on the footprint"
        _assert_scale_kept_and_words_cleared(qs, am, "fp8 forward, " + what)


@pytest.mark.parametrize("M,N,K,cfg", [(257, 264, 1024, 20)])
def test_gemm_fp8_data_gradient_footprint_and_copy(M, N, K, cfg):
    """e5m2 A x e4m3 B with the e5m2 copy: an e5m2 NaN in A and an e4m3 NaN byte in B; q_out decodes to NaN on the footprint (the copy
    of a NaN is a NaN, never the saturated -57344).  An e5m2 inf byte (0x7C) in A: its row of y is +-inf, and its copy saturates to
    +-57344 (bytes 0x7B / 0xFB) with amax = inf -- the existing saturation rule."""
    qa, qb = GR.operands(M, N, K, 8, 16, seed=M + N, kind="e5m2", kind_b="e4m3")
    sa_d, sb_d = torch.tensor([2.0], device=DEV), torch.tensor([16.0], device=DEV)

    def run(qa, qb):
        q_out = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
        qs, am = _fp8_words()
        y, recs = _logged(lambda: ops.gemm_fp8(_f8(qa, "e5m2"), _f8(qb, "e4m3"), sa_d, sb_d, M, N, K, a_bf8=True, q_bf8=True, q_out=q_out,
                                               q_scale=qs, q_amax=am))
        assert recs == [(cfg, 1, 1)], recs
        return dict(y=y, q=q_out.view(torch.float8_e5m2)), qs, am

    def ref(qa, qb):
        r = GR.epilogue(GR.ref_nt(qa, qb), alpha=1.0 / 32, q_scale=0.25, q_kind="e5m2")
        return dict(y=r["y"], q=r["q"])
    clean, _, _ = run(qa, qb)
    pois = (PR.plant(qa, (0, 0), NAN), PR.plant(qb, (N - 1, K - 1), NAN))
    got, qs, am = run(*pois)
    F = PR.footprint(ref, (qa, qb), pois)
    assert int(F["y"].sum()) == M + N - 1
    PR.assert_footprint(clean, got, F, "fp8 data gradient")
    assert bool(torch.isnan(got["q"].float().cpu()[F["q"]]).all()), "the e5m2 copy of a NaN must be a NaN"
    _assert_scale_kept_and_words_cleared(qs, am, "fp8 data gradient")
    pa = PR.plant(qa, (0, 0), INF)
    assert int(_f8(pa, "e5m2").view(torch.uint8)[0, 0]) == 0x7C
    got, qs, am = run(pa, qb)
    PR.assert_footprint(clean["y"], got["y"], PR.footprint(lambda x, y: ref(x, y)["y"], (qa, qb), (pa, qb)), "fp8 data gradient, inf in A")
    assert bool(torch.isinf(got["y"][0].float()).all()) and set((got["q"].view(torch.uint8)[0] & 0x7F).tolist()) == {0x7B}
    assert torch.equal(got["q"].view(torch.uint8)[1:], clean["q"].view(torch.uint8)[1:]) and float(am.max()) == INF


@pytest.mark.parametrize("tile", (36, 37))
def test_gemm_fp8_weight_gradient_footprint(tile):
    """dW (+)= dy^T x from e5m2 / e4m3 token-major operands, single (R = 129) and a group of 8: an e5m2 inf in dy(r, n) poisons row n, an
    e4m3 NaN in x(r, k) column k; the other problems of the group keep their bits."""
    R = 129
    sd_d, sx_d = torch.tensor([4.0], device=DEV), torch.tensor([8.0], device=DEV)
    shapes = ((144, 208), (16, 16), (272, 48), (64, 1040), (48, 336), (768, 64), (128, 128), (32, 80))
    data = [(GR.ints((R, N), 8, 50 + i, "e5m2"), GR.ints((R, K), 16, 60 + i, "e4m3"), GR.unit_ints((N, K), 64, 70 + i, 1.0 / 32))
            for i, (N, K) in enumerate(shapes)]

    def run(items):
        probs = [(_f8(dq, "e5m2"), _f8(xq, "e4m3"), sd_d, sx_d, pre.float().to(DEV)) for dq, xq, pre in items]
        _, recs = _logged(lambda: ops.gemm_wgrad_fp8(probs, accumulate=True, tile=tile))
        assert recs == [(tile, 1, len(items))], recs
        return [p[4] for p in probs]

    def ref(*flat):
        return tuple(GR.f32(GR.ref_tt(flat[3 * i], flat[3 * i + 1]) / 32 + flat[3 * i + 2]) for i in range(len(flat) // 3))
    for items, j in ((data[:1], 0), (data, 3)):
        clean = run(items)
        pois = list(items)
        N, K = shapes[j]
        pois[j] = (PR.plant(items[j][0], (R - 1, N - 1), INF), PR.plant(items[j][1], (0, 0), NAN), items[j][2])
        F = PR.footprint(ref, [t for d in items for t in d], [t for d in pois for t in d])
        assert [int(f.sum()) for f in F] == [(N + K - 1) if i == j else 0 for i in range(len(items))]
        PR.assert_footprint(clean, run(pois), F, "fp8 weight gradient cfg %d, %d problems" % (tile, len(items)))


# ------------------------------------------------------------------------------------------- fp8 copies and their amax
@pytest.mark.parametrize("n", [8, 8 * 257])
def test_fp8_quantize_bf16_copies_nan_and_reports_it(n):
    """A cast is a pure function of one element: the bytes are torch's, a NaN's byte is the NaN byte, -inf saturates to 0xFE."""
    x = (rand(n, scale=2.0, seed=n) * 30).cpu()
    x[n - 1], x[0] = NAN, -INF
    xb = bf(torch.cat([x, torch.full((PAD,), NAN)]).to(DEV))[:n]
    q = torch.zeros(n + 8, device=DEV, dtype=torch.uint8)
    sc, am = torch.tensor([17.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    ops.fp8_quantize_bf16(xb, q[:n], sc, am)
    want = GR.e4m3(xb.double().cpu() * 17.0)
    got = q[:n].view(torch.float8_e4m3fn).double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[n - 1]))
    assert torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
    assert int(q[0]) == 0xFE and int(q[n:].max()) == 0
    _assert_scale_kept_and_words_cleared(sc, am, "fp8_quantize_bf16")
    # inf alone: the maximum is inf (the existing saturation rule), no NaN needed
    x[n - 1] = 1.0
    am.zero_()
    ops.fp8_quantize_bf16(bf(x.to(DEV)), q[:n], sc, am)
    assert float(am.max()) == INF


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_fp8_amax_words_report_a_nan(n):
    """The amax side alone (no byte is looked at): a NaN anywhere in the tensor is in the amax words after the launch -- fmaxf and a
    float compare would both drop it -- and crct_fp8_update_scales then keeps the scale and clears the words."""
    x = (rand(n, scale=2.0, seed=n + 1)).cpu()
    x[n // 2] = NAN
    sc, am = torch.tensor([17.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    ops.fp8_quantize_bf16(bf(x.to(DEV)), torch.zeros(n, device=DEV, dtype=torch.uint8), sc, am)
    _assert_scale_kept_and_words_cleared(sc, am, "fp8_quantize_bf16, amax")


@pytest.mark.parametrize("M,H", [(7, 96), (255, 520)])
def test_layernorm_fp8_copies_carry_the_nan(M, H):
    """crct_layernorm_fwd_q (e4m3 copy of y) and CrctLnBwdArgs.q_out (e5m2 copy of the gradient): the NaN row's bytes decode to NaN,
    the other rows' bytes are the clean launch's, the amax words hold NaN."""
    lib = L.load()
    x = (rand(M, H, scale=2.0, seed=M) + 0.3).cpu().double()
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3)
    r = M // 2

    def fwd(x):
        xb = bf(_nan_rows(x))[:M]
        y, yq = torch.empty(M, H, device=DEV, dtype=torch.bfloat16), torch.zeros(M, H, device=DEV, dtype=torch.uint8)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        sc, am = torch.tensor([30.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
        L.check(lib.crct_layernorm_fwd_q(xb.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         M, H, 1e-12, 0, 1.0, 0, 0, yq.data_ptr(), sc.data_ptr(), am.data_ptr(), L.current_stream()))
        return dict(y=y, q=yq.view(torch.float8_e4m3fn), mean=mean, rstd=rstd), sc, am
    rows = torch.zeros(M, dtype=torch.bool)
    rows[r] = True
    F = dict(y=rows[:, None].expand(M, H), q=rows[:, None].expand(M, H), mean=rows, rstd=rows)
    clean, _, am = fwd(x)
    assert torch.equal(clean["y"], ops.layernorm_fwd(bf(x.to(DEV)), gamma, beta)[0]) and bool(torch.isfinite(am).all())
    got, sc, am = fwd(PR.plant(x, (r, H - 1), NAN))
    PR.assert_footprint(clean, got, F, "layernorm_fwd_q")
    assert bool(((got["q"].view(torch.uint8)[r] & 0x7F) == 0x7F).all())
    _assert_scale_kept_and_words_cleared(sc, am, "layernorm_fwd_q")

    dy = (rand(M, H, scale=2e-3, seed=4)).cpu().double()
    xb = bf(x.to(DEV))
    mean, rstd = clean["mean"], clean["rstd"]

    def bwd(dy):
        a = L.LnBwdArgs()
        dyb = bf(_nan_rows(dy))[:M]
        dx, q = torch.empty(M, H, device=DEV, dtype=torch.bfloat16), torch.zeros(M, H, dtype=torch.uint8, device=DEV)
        part = torch.empty(3 * 4 * lib.crct_layernorm_bwd_blocks(M) * H, device=DEV)
        qs, am = torch.tensor([4096.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
        a.dy, a.x, a.mean, a.rstd, a.gamma, a.dx, a.partials = (L.ptr(t) for t in (dyb, xb, mean, rstd, gamma, dx, part))
        a.M, a.H, a.post_thr, a.post_scale, a.lin_thr, a.lin_scale = M, H, 0, 1.0, 0, 1.0
        a.q_out, a.q_scale, a.q_amax = L.ptr(q), L.ptr(qs), L.ptr(am)
        L.check(lib.crct_layernorm_bwd_rows_args(C.byref(a), L.current_stream()), "layernorm_bwd_rows_args")
        return dict(dx=dx, q=q.view(torch.float8_e5m2)), qs, am
    clean, _, am = bwd(dy)
    assert bool(torch.isfinite(am).all())
    got, qs, am = bwd(PR.plant(dy, (r, 0), NAN))
    PR.assert_footprint(clean, got, dict(dx=F["y"], q=F["q"]), "CrctLnBwdArgs.q_out")
    assert bool(torch.isnan(got["q"].float()[r]).all())
    _assert_scale_kept_and_words_cleared(qs, am, "CrctLnBwdArgs.q_out")


# ------------------------------------------------------------------------------------------- LayerNorm, softmax, column sums
_LN_SHAPES = [(7, 96), (255, 520), (7, 2048)]


def _ln64(x, gamma, beta):
    mean, _, rstd = _ln_stats64(x)
    return dict(y=gamma * ((x - mean[:, None]) * rstd[:, None]) + beta, mean=mean, rstd=rstd)


@pytest.mark.parametrize("f32_rows", [False, True])
@pytest.mark.parametrize("M,H", _LN_SHAPES)
def test_layernorm_forward_footprint(M, H, f32_rows):
    x = GR.bf16((rand(M, H, scale=2.0, seed=M + H) + 0.3).cpu())
    gamma, beta = 1 + 0.1 * rand(H, seed=2), 0.1 * rand(H, seed=3)

    def run(x):
        buf = _nan_rows(x)
        y, mean, rstd = ops.layernorm_fwd((buf.float() if f32_rows else bf(buf))[:M], gamma, beta)
        return dict(y=y, mean=mean, rstd=rstd)
    clean = run(x)
    _check_ln_forward_terms(x, clean["y"], clean["mean"], clean["rstd"], gamma, beta, "layernorm_fwd: clean launch from NaN-padded rows")
    for r, c, val in ((M - 1, H - 1, NAN), (0, 0, INF), (M // 2, H // 2, -INF)):
        xp = PR.plant(x, (r, c), val)
        F = PR.footprint(lambda t: _ln64(t, gamma.double().cpu(), beta.double().cpu()), (x,), (xp,))
        assert int(F["y"].sum()) == H and int(F["mean"].sum()) == 1 and int(F["rstd"].sum()) == 1 and bool(F["y"][r].all())
        PR.assert_footprint(clean, run(xp), F, "layernorm_fwd %dx%d %s at (%d, %d)" % (M, H, "fp32" if f32_rows else "bf16", r, c))


@pytest.mark.parametrize("f32_rows", [False, True])
@pytest.mark.parametrize("M,H", _LN_SHAPES)
def test_layernorm_backward_footprint(M, H, f32_rows):
    """NaN in dy(r, c): row r of dx and dx_lin, column c of dgamma / dbeta, and -- dx row r summed over the rows -- all of dbias.  NaN in x(r, c)
    (with the statistics the forward gave for it): row r of dx, all of dgamma and dbias, none of dbeta (a sum over dy alone)."""
    x = GR.bf16((rand(M, H, scale=2.0, seed=M + H) + 0.3).cpu())
    dy = GR.bf16(rand(M, H, seed=4).cpu())
    gamma = 1 + 0.1 * rand(H, seed=2)

    def run(x, dy):
        xin = (_nan_rows(x).float() if f32_rows else bf(_nan_rows(x)))[:M]
        _, mean, rstd = ops.layernorm_fwd(xin, gamma, torch.zeros_like(gamma))
        dx, dxl, dg, db, dbias = ops.layernorm_bwd(bf(_nan_rows(dy))[:M], xin, mean, rstd, gamma, want_lin=True)
        return dict(dx=dx, dx_lin=dxl, dgamma=dg, dbeta=db, dbias=dbias)

    def ref(x, dy):
        # a fresh leaf per call: _ln_backward64 makes an fp64 CPU tensor itself the leaf, whose .grad would accumulate over the calls
        ds, dg, db, _, _ = _ln_backward64(x.detach().clone(), dy, torch.ones(M, H, dtype=torch.float64), gamma)
        return dict(dx=ds, dx_lin=ds, dgamma=dg, dbeta=db, dbias=ds.sum(0))       # no lin dropout: dx_lin = dx
    clean = run(x, dy)
    xd = x.to(DEV).float() if f32_rows else bf(x.to(DEV))       # R4: the clean launch from NaN-padded rows against fp64, at the existing budget
    _, mean_c, rstd_c = ops.layernorm_fwd(xd, gamma, torch.zeros_like(gamma))
    _ln_check_backward(xd, bf(dy.to(DEV)), mean_c, rstd_c, gamma, None, 0.0, None, 0.0,
                       (clean["dx"], clean["dx_lin"], clean["dgamma"], clean["dbeta"], clean["dbias"]), "layernorm_bwd: clean launch")
    assert torch.equal(clean["dx_lin"], clean["dx"])             # no lin dropout
    r, c = M - 1, H - 1
    for what, pois, counts in (("dy", (x, PR.plant(dy, (r, c), NAN)), dict(dx=H, dx_lin=H, dgamma=1, dbeta=1, dbias=H)),
                               ("x", (PR.plant(x, (r, c), NAN), dy), dict(dx=H, dx_lin=H, dgamma=H, dbeta=0, dbias=H))):
        F = PR.footprint(ref, (x, dy), pois)
        assert {k: int(v.sum()) for k, v in F.items()} == counts, (what, {k: int(v.sum()) for k, v in F.items()})
        PR.assert_footprint(clean, run(*pois), F, "layernorm_bwd %dx%d, NaN in %s" % (M, H, what))


def test_softmax_rows_footprint():
    M, Fw = 15, 132
    x = GR.bf16((rand(M, Fw, scale=3.0, seed=1)).cpu())
    g = GR.f32(rand(M, Fw, seed=2).cpu())
    for dtype in (torch.bfloat16, torch.float32):
        def run(x, g):
            xin = _nan_rows(x).to(dtype)[:M]
            return dict(y=ops.softmax_rows(xin), dx=ops.softmax_bwd_rows(xin, _nan_rows(g).float()[:M]))

        def ref(x, g):
            y = torch.softmax(x, -1)
            return dict(y=y, dx=y * (g - (y * g).sum(-1, keepdim=True)))
        clean = run(x, g)
        ref_c = ref(x, g)
        _assert_within_bf16_step(clean["y"], ref_c["y"], ref_c["y"], "softmax_rows: clean launch")
        r_bwd = IG.ratio(clean["dx"], IG.softmax_bwd_reference(x.float(), g.float()), IG.softmax_bwd_budget(x.float(), g.float()))
        assert float(r_bwd.max()) <= 1.0, ("softmax_bwd_rows: clean launch", float(r_bwd.max()))
        for what, pois, counts in (("NaN in x", (PR.plant(x, (M - 1, Fw - 1), NAN), g), dict(y=Fw, dx=Fw)),
                                   ("+inf in x", (PR.plant(x, (0, 0), INF), g), dict(y=Fw, dx=Fw)),
                                   ("NaN in g", (x, PR.plant(g, (7, 64), NAN)), dict(y=0, dx=Fw))):
            F = PR.footprint(ref, (x, g), pois)
            assert {k: int(v.sum()) for k, v in F.items()} == counts, (what, {k: int(v.sum()) for k, v in F.items()})
            PR.assert_footprint(clean, run(*pois), F, "softmax rows %s, %s" % (dtype, what))


def test_colsum_footprint():
    M, N, ld = 255, 520, 528
    x = GR.ints((M, N), 255, M + N)
    pre = GR.ints((N,), 255, 3)

    def run(x):
        xb = bf(_nan_rows(x, ld))
        out = pre.float().to(DEV)
        ops.colsum(xb, M, N, ld=ld, out=out, accumulate=True)
        return dict(fresh=ops.colsum(xb, M, N, ld=ld), acc=out)

    def ref(x):
        return dict(fresh=x.sum(0), acc=x.sum(0) + pre)
    clean = run(x)
    for k, v in ref(x).items():
        _assert_bits(clean[k], v, "colsum clean: " + k)
    for r, c in ((M - 1, N - 1), (0, 0), (128, 519)):
        xp = PR.plant(x, (r, c), NAN)
        F = PR.footprint(ref, (x,), (xp,))
        assert int(F["fresh"].sum()) == 1 and bool(F["fresh"][c])
        PR.assert_footprint(clean, run(xp), F, "colsum, NaN at (%d, %d)" % (r, c))


# ------------------------------------------------------------------------------------------- attention
ATT_GUARD = 32                 # NaN rows behind q / k / v / dctx: one key-tile pair of the long kernels


class _AttnCase:
    """q, k, v, dctx as column slices of fused buffers whose other columns, and ATT_GUARD rows behind the last batch element, are NaN.
    Batch 0 has masked keys; batch 1 (the poisoned one) attends every key: what a masked key row does to 0 * NaN is no contract."""

    def __init__(self, B, heads, Tq, Tk, d, seed):
        self.B, self.heads, self.Tq, self.Tk, self.d, self.H = B, heads, Tq, Tk, d, heads * d
        g = torch.Generator().manual_seed(seed)
        H = self.H
        self.t = dict(q=AR.bf16(torch.randn(B, Tq, H, generator=g)), k=AR.bf16(torch.randn(B, Tk, H, generator=g)),
                      v=AR.bf16(torch.randn(B, Tk, H, generator=g)), dctx=AR.bf16(torch.randn(B, Tq, H, generator=g)))
        km = torch.ones(B, Tk, dtype=torch.uint8)
        km[0, Tk // 2:] = 0
        self.km = km
        self._ref = {}

    def _fused(self, x, T, ld, c0):
        flat = torch.full((self.B * T + ATT_GUARD, ld), NAN, dtype=torch.float64)
        flat[:self.B * T, c0:c0 + self.H] = x.reshape(self.B * T, self.H)
        return bf(flat.to(DEV))[:self.B * T].view(self.B, T, ld)[:, :, c0:c0 + self.H]

    def _canvas(self, T, ld, c0):
        flat = torch.full((self.B * T + 3, ld), NAN, device=DEV, dtype=torch.bfloat16)
        return flat, flat[:self.B * T].view(self.B, T, ld)[:, :, c0:c0 + self.H]

    def run(self, t, kept=False, lse_poison=None, ignored_lse=False):
        B, heads, Tq, Tk, d, H = self.B, self.heads, self.Tq, self.Tk, self.d, self.H
        q, k, v, do = (self._fused(t["q"], Tq, 3 * H + 8, 0), self._fused(t["k"], Tk, 3 * H + 8, H), self._fused(t["v"], Tk, 3 * H + 8, 2 * H),
                       self._fused(t["dctx"], Tq, H + 8, 8))
        km = self.km.to(DEV)
        fc, ctx = self._canvas(Tq, H + 8, 0)
        fq, dq = self._canvas(Tq, 3 * H, 0)
        fk, dk = self._canvas(Tk, 3 * H, H)
        dv = fk[:B * Tk].view(B, Tk, 3 * H)[:, :, 2 * H:]
        lse = torch.full((B, heads, Tq), NAN, device=DEV) if kept or ignored_lse else None
        ops.attention_fwd(q, k, v, km, heads, d, row_lse=lse, out=ctx)
        if lse_poison is not None:
            lse[lse_poison] = NAN
        ops.attention_bwd(q, k, v, km, do, heads, d, row_lse=lse, ctx=ctx if kept or ignored_lse else None, outs=(dq, dk, dv))
        if ignored_lse:        # R4: the short kernels recompute their statistics; a row_lse handed to them is neither written nor read
            assert bool(torch.isnan(lse).all()), "a kernel that recomputes its statistics wrote row_lse"
        for flat, c0, c1, T, what in ((fc, 0, H, Tq, "ctx"), (fq, 0, H, Tq, "dq"), (fk, H, 3 * H, Tk, "dk / dv")):
            mask = torch.ones(flat.shape, dtype=torch.bool, device=DEV)
            mask[:B * T, c0:c1] = False
            assert bool(torch.isnan(flat[mask]).all()), "attention %s canvas: elements outside the output slice were written" % what
        return dict(ctx=ctx.clone(), dq=dq.clone(), dk=dk.clone(), dv=dv.clone())

    def ref(self, t):
        r = AR.reference(t["q"], t["k"], t["v"], self.km, t["dctx"], self.heads, self.d)
        return {n: r[n] for n in AR.OUTPUTS}

    def head(self, b, h, T, rows=None):
        """bool [B, T, H]: head h of batch b (rows: these rows only)."""
        m = torch.zeros(self.B, T, self.H, dtype=torch.bool)
        m[b, slice(None) if rows is None else rows, h * self.d:(h + 1) * self.d] = True
        return m

    def check(self, tag, kept=False, ignored_lse=False):
        """One NaN at a time at the sites of the issue, in an attended position of batch 1, head 1."""
        B, Tq, Tk, d = self.B, self.Tq, self.Tk, self.d
        assert B == 2 and self.heads >= 2
        clean = self.run(self.t, kept)
        if ignored_lse:
            got = self.run(self.t, ignored_lse=True)
            for n in AR.OUTPUTS:
                assert torch.equal(PR.bits(got[n]), PR.bits(clean[n])), "%s: %s changes when a NaN-filled row_lse is handed over" % (tag, n)
        if ("clean", kept) not in self._ref:
            r = AR.reference(self.t["q"], self.t["k"], self.t["v"], self.km, self.t["dctx"], self.heads, d,
                             ctx_bf16=clean["ctx"].cpu() if kept else None)
            self._ref["clean", kept] = r
        r = self._ref["clean", kept]
        for n in AR.OUTPUTS:       # R4: the clean launch from NaN-surrounded operands is still within the fp64 budget
            AR.assert_within(clean[n].cpu(), r[n], AR.budget_of(r, n, kept), "%s: clean %s" % (tag, n))
        i, j, c = Tq - 1, max(Tk - 2, 0), d + d - 1
        none = torch.zeros(B, Tq, self.H, dtype=torch.bool)
        col = torch.zeros(B, Tk, self.H, dtype=torch.bool)      # dv(j, c) = sum_i Pd(i, j) dctx(i, c): column c of every key row
        col[1, :, c] = True
        sites = [("q", (1, i, d), dict(ctx=self.head(1, 1, Tq, i), dq=self.head(1, 1, Tq, i), dk=self.head(1, 1, Tk), dv=self.head(1, 1, Tk))),
                 ("k", (1, j, c), dict(ctx=self.head(1, 1, Tq), dq=self.head(1, 1, Tq), dk=self.head(1, 1, Tk), dv=self.head(1, 1, Tk))),
                 ("v", (1, j, c), None),
                 ("dctx", (1, i, c), dict(ctx=none, dq=self.head(1, 1, Tq, i), dk=self.head(1, 1, Tk), dv=col))]
        for name, idx, want in sites:
            tp = dict(self.t)
            tp[name] = PR.plant(self.t[name], idx, NAN)
            F = PR.footprint(self.ref, (self.t,), (tp,))
            if want is not None:
                for n in AR.OUTPUTS:
                    assert torch.equal(F[n], want[n]), (tag, name, n, int(F[n].sum()), int(want[n].sum()))
            else:                  # v(j, c): column c of every query row's ctx in the (batch, head); dP, so all of dq / dk; none of dv
                assert int(F["ctx"].sum()) == Tq and int(F["dv"].sum()) == 0 and torch.equal(F["dq"], self.head(1, 1, Tq))
            PR.assert_footprint(clean, self.run(tp, kept), F, "%s: NaN in %s%s" % (tag, name, idx))
        if kept:
            # A NaN in the kept row_lse(1, 1, i), planted between forward and backward.  The kept form takes P(i, :) = exp2(x - lse(i))
            # (attention_ref.py, emulate): that row of P is NaN, so dq(i), and through P^T / dS^T all of dk and dv of the (batch, head).
            F = dict(ctx=none, dq=self.head(1, 1, Tq, i), dk=self.head(1, 1, Tk), dv=self.head(1, 1, Tk))
            PR.assert_footprint(clean, self.run(self.t, kept, lse_poison=(1, 1, i)), F, "%s: NaN in row_lse" % tag)


@pytest.mark.parametrize("tag,hooks,shape,kept", [
    ("valu", dict(valu=1), (2, 3, 5, 17, 24), False),
    ("mfma split 1", dict(split=1), (2, 3, 5, 17, 32), False),
    ("mfma split 2", dict(split=2), (2, 3, 36, 36, 48), False),
    ("mfma split 0", dict(split=0), (2, 3, 49, 65, 64), False),
    ("long forced", dict(long=1), (2, 2, 5, 5, 48), False),
    ("long forced, kept", dict(long=1), (2, 2, 20, 36, 32), True),
    ("long", dict(), (2, 2, 113, 113, 32), False),
    ("long, kept", dict(), (2, 2, 129, 17, 48), True),
    ("d = 128", dict(), (2, 2, 17, 36, 128), False),
    ("d = 128, split 1", dict(split=1), (2, 2, 5, 17, 128), False),
    ("d = 128 long, kept", dict(), (2, 2, 124, 44, 128), True),
], ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) else None)
def test_attention_footprint(tag, hooks, shape, kept):
    case = _AttnCase(*shape, seed=sum(shape))
    with _hooks(**hooks):
        case.check(tag, kept=kept, ignored_lse=not kept and not tag.startswith("long") and shape[4] != 128)


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(2, 3, 17, 36, 32), (2, 2, 124, 44, 128)])
def test_attention_probs_footprint(B, heads, Tq, Tk, d):
    """crct_attention_probs (fp32 maps [B, heads, Tq, Tk]) from NaN-surrounded q / k slices into a NaN-guarded buffer: a NaN in q(1, i)
    of head 1 poisons that row of that map, one in k(1, j) every row of it; batch 0 and the other heads keep their bits."""
    import attention_probs_ref as APR
    case = _AttnCase(B, heads, Tq, Tk, d, seed=Tq + Tk)
    H = case.H

    def run(t):
        q, k = case._fused(t["q"], Tq, 3 * H + 8, 0), case._fused(t["k"], Tk, 3 * H + 8, H)
        flat = torch.full((B * heads * Tq * Tk + 67,), NAN, device=DEV)
        out = flat[:B * heads * Tq * Tk].view(B, heads, Tq, Tk)
        ops.attention_probs(q, k, case.km.to(DEV), heads, d, out=out)
        assert bool(torch.isnan(flat[B * heads * Tq * Tk:]).all()), "attention_probs wrote past its output"
        return out.clone()

    def ref(t):
        return APR.reference(t["q"], t["k"], case.km, heads, d)
    clean = run(case.t)
    APR.assert_within(clean.cpu(), *ref(case.t), "attention_probs: clean launch")
    for name, idx, rows in (("q", (1, Tq - 1, d), slice(Tq - 1, Tq)), ("k", (1, Tk - 2, 2 * d - 1), slice(None))):
        tp = dict(case.t)
        tp[name] = PR.plant(case.t[name], idx, NAN)
        F = PR.footprint(lambda t: ref(t)[0], (case.t,), (tp,))
        want = torch.zeros(B, heads, Tq, Tk, dtype=torch.bool)
        want[1, 1, rows] = True
        assert torch.equal(F, want), name
        PR.assert_footprint(clean, run(tp), F, "attention_probs, NaN in %s%s" % (name, idx))


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(2, 16, 20, 36, 64), (2, 16, 124, 124, 48), (2, 2, 36, 36, 128)])
def test_attention_fp8_copies_carry_the_nan(B, heads, Tq, Tk, d):
    """crct_attention_fwd_q / _bwd_q: the e4m3 copy of ctx and the e5m2 copies of dq / dk / dv decode to NaN exactly where their bf16
    twins are NaN, keep the clean launch's bytes elsewhere, and the amax words hold NaN."""
    case = _AttnCase(B, heads, Tq, Tk, d, seed=Tq + d)
    km = case.km.to(DEV)

    def run(t):
        q, k, v, do = (bf(t[n].to(DEV)) for n in ("q", "k", "v", "dctx"))
        sc = [torch.tensor([s], device=DEV) for s in (16.0, 64.0, 64.0)]
        am = [torch.zeros(L.FP8_AMAX_LANES, device=DEV) for _ in range(3)]
        ctx, ctx8 = ops.attention_fwd_q(q, k, v, km, heads, d, sc[0], am[0])
        (dq, dk, dv), (dq8, dk8, dv8) = ops.attention_bwd_q(q, k, v, km, do, heads, d, sc[1], am[1], sc[2], am[2])
        out = dict(ctx=ctx, dq=dq, dk=dk, dv=dv, ctx8=ctx8.view(torch.float8_e4m3fn), dq8=dq8.view(torch.float8_e5m2),
                   dk8=dk8.view(torch.float8_e5m2), dv8=dv8.view(torch.float8_e5m2))
        return out, sc, am
    clean, _, am = run(case.t)
    assert all(bool(torch.isfinite(a).all()) for a in am)
    tp = dict(case.t)
    tp["q"] = PR.plant(case.t["q"], (1, Tq - 1, d), NAN)
    got, sc, am = run(tp)
    F = PR.footprint(case.ref, (case.t,), (tp,))
    F.update({n + "8": F[n] for n in AR.OUTPUTS})
    PR.assert_footprint(clean, got, F, "attention fp8 copies")
    for n in AR.OUTPUTS:
        assert bool(torch.isnan(got[n + "8"].float().cpu()[F[n]]).all()), n + ": the fp8 copy of a NaN must be a NaN"
    for s, a, what in zip(sc, am, ("ctx", "dq", "dk / dv")):
        _assert_scale_kept_and_words_cleared(s, a, "attention amax of " + what)


# ------------------------------------------------------------------------------------------- the e4m3 weight shadow
def _nan_byte(b):
    return (b & 0x7F) == 0x7F


def test_fp8_weight_shadow_carries_a_nan_weight():
    """A NaN weight in a shadowed tensor (optim_ref.shadow_fixture): crct_fp8_quantize_weights and the CrctFp8Shadow of
    crct_adamw_step write the NaN byte for it (never the saturated 0xFE), its slot's amax words hold NaN until
    crct_fp8_update_scales meets them (the scale stays, the words are cleared), and every other byte, word and scale is the
    clean launch's."""
    from test_optim_gpu import LANES, _Shadow, _q8_torch
    sh = _Shadow()
    fx, lay = sh.fx, sh.lay
    seg = next(i for i, s in enumerate(fx["slot"]) if s >= 0 and fx["seg_in"][i] > 0)      # a weight with a transposed copy
    slot, at = fx["slot"][seg], fx["off"][seg] + 5
    same_slot = torch.zeros(fx["total"], dtype=torch.bool)
    for o, n, s in zip(fx["off"], fx["len"], fx["slot"]):
        if s == slot:
            same_slot[o:o + n] = True
    # ---- start-up quantisation
    prev = [5.0 + i for i in range(fx["n_slots"])]
    res = {}
    for name in ("clean", "poisoned"):
        p = fx["p"].clone()
        if name == "poisoned":
            p[at] = NAN
        scale = torch.tensor(prev, device=DEV)
        amax = torch.full((fx["n_slots"] * LANES,), 3.0, device=DEV)
        q = torch.full((fx["total"],), 0x55, dtype=torch.uint8, device=DEV)
        ops.fp8_quantize_weights(lay.padded(p, fill=NAN).to(DEV), q, lay.seg_off, lay.seg_len, sh.seg_slot, lay.blk_seg, lay.blk_off, scale, amax)
        torch.cuda.synchronize()
        res[name] = (q.cpu(), scale.cpu(), amax.cpu().view(fx["n_slots"], LANES), p)
    (qc, sc, ac, _), (qp, sp, ap, pp) = res["clean"], res["poisoned"]
    assert bool(_nan_byte(qp[at])) and int(_nan_byte(qp).sum()) == 1 and not bool(_nan_byte(qc).any())
    assert torch.equal(qp[~same_slot], qc[~same_slot]), "quantize_weights: bytes of the other slots changed"
    others = [s for s in range(fx["n_slots"]) if s != slot]
    assert float(sp[slot]) == prev[slot] and torch.equal(sp[others], sc[others]), "quantize_weights: the NaN slot keeps its scale, the others theirs"
    assert bool(torch.isfinite(ap).all()) and float(ap[slot].abs().max()) == 0.0, "quantize_weights: the NaN slot's words are cleared"
    want = _q8_torch(pp[same_slot], prev[slot])            # the slot's other bytes: quantised with the scale that was kept
    keep = ~_nan_byte(want)
    assert torch.equal(qp[same_slot][keep], want[keep]) and int((~keep).sum()) == 1
    # ---- the update's shadow
    res = {}
    for name in ("clean", "poisoned"):
        st = sh.fresh()
        if name == "poisoned":
            st.p[at] = NAN
        st.launch(lay.padded(fx["g"]).to(DEV), 1, fp8=st.f8, max_workgroups=2)
        res[name] = st
    c, p = res["clean"], res["poisoned"]
    elem = torch.zeros(fx["total"], dtype=torch.bool, device=DEV)
    elem[at] = True
    inside = fx["inside"].to(DEV)
    F = dict(p=elem, pb=elem, q=elem)
    def inner(st):             # the sentinels between the tensors are not outputs (tests/test_optim_gpu.py checks that they stay)
        zero8 = torch.zeros((), dtype=torch.uint8, device=DEV)
        return dict(p=torch.where(inside, st.p, 0.0), pb=torch.where(inside, st.pb, 0.0), q=torch.where(inside, st.q, zero8).view(torch.float8_e4m3fn))
    PR.assert_footprint(inner(c), inner(p), F, "crct_adamw_step with CrctFp8Shadow")
    for n in ("m", "v"):
        assert torch.equal(PR.bits(getattr(p, n)), PR.bits(getattr(c, n))), n + " depends on the gradient alone"
    dq = p.qt != c.qt
    assert int(dq.sum()) == 1 and bool(_nan_byte(p.qt[dq]).all()), "the transposed shadow: one byte differs, and it is the NaN byte"
    wc, wp = c.amax.view(fx["n_slots"], LANES), p.amax.view(fx["n_slots"], LANES)
    assert bool(torch.isnan(wp[slot]).any()) and torch.equal(wp[others], wc[others]) and bool(torch.isfinite(wc).all())
    before = p.scale.clone()
    ops.fp8_update_scales(p.scale, p.amax, n=fx["n_slots"])
    assert float(p.scale[slot]) == float(before[slot]) and float(wp[slot].abs().max()) == 0.0 and bool(torch.isfinite(p.scale).all())


# ------------------------------------------------------------------------------------------- the sequence-output row kernels
def test_layernorm_rows_f32_and_hidden_grad_add_keep_a_nan_to_its_row():
    """crct_layernorm_rows_f32 (a NaN in the source row, in mean[r] or in rstd[r]: row r of the rebuilt output) and
    crct_hidden_grad_add (x += c g in place: element by element, so a NaN of g reaches its own element), rows behind M NaN."""
    lib = L.load()
    M, N, r = 5, 96, 3
    s = GR.f32((rand(M, N, scale=1.7, seed=1) + 0.3).cpu())
    gamma, beta = (1 + 0.2 * rand(N, seed=2)).cpu().double(), (0.1 * rand(N, seed=3)).cpu().double()
    mean, _, rstd = _ln_stats64(s)
    mean, rstd = GR.f32(mean), GR.f32(rstd)

    def run(s, mean, rstd):
        sd = _nan_rows(s, pad=16).float()
        vec = [torch.cat([t.float(), torch.full((16,), NAN)]).to(DEV) for t in (mean, rstd, gamma, beta)]
        out = torch.full((M * N + 32,), NAN, device=DEV)
        L.check(lib.crct_layernorm_rows_f32(sd.data_ptr(), 0, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(),
                                            out.data_ptr(), M, N, L.current_stream()), "layernorm_rows_f32")
        assert bool(torch.isnan(out[M * N:]).all()), "layernorm_rows_f32 wrote past the last row"
        return out[:M * N].view(M, N).clone()

    def ref(s, mean, rstd):
        return gamma * ((s - mean[:, None]) * rstd[:, None]) + beta
    clean_in = (s, mean, rstd)
    clean = run(*clean_in)
    for i, idx in ((0, (r, N - 1)), (1, r), (2, r)):
        pois = list(clean_in)
        pois[i] = PR.plant(clean_in[i], idx, NAN)
        F = PR.footprint(ref, clean_in, pois)
        assert int(F.sum()) == (1 if i == 0 else N)           # the statistics are inputs here: a NaN element of s stays an element
        PR.assert_footprint(clean, run(*pois), F, "layernorm_rows_f32, NaN in input %d" % i)

    n = M * N
    x = GR.bf16((rand(n, scale=0.05, seed=4)).cpu())
    g = GR.f32(rand(n, scale=0.05, seed=5).cpu())

    def add(g):
        xd = bf(torch.cat([x, torch.full((32,), NAN, dtype=torch.float64)]).to(DEV))
        gd = torch.cat([g, torch.full((32,), NAN, dtype=torch.float64)]).float().to(DEV)
        L.check(lib.crct_hidden_grad_add(xd.data_ptr(), gd.data_ptr(), 0.5, n, L.current_stream()), "hidden_grad_add")
        assert bool(torch.isnan(xd[n:]).all())
        return xd[:n].clone()
    clean = add(g)
    _assert_bits(clean, GR.bf16(x + 0.5 * g), "hidden_grad_add: clean")
    gp = PR.plant(PR.plant(g, n - 1, NAN), 0, INF)
    PR.assert_footprint(clean, add(gp), PR.footprint(lambda t: x + 0.5 * t, (g,), (gp,)), "hidden_grad_add")


# ------------------------------------------------------------------------------------------- embeddings
# The embedding kernels at the smallest multi-row cases of tests/test_kernels_gpu.py's tables: text (B, T) = (3, 7), H = 64, p = 0.1 and
# image M = 7, H = 64, p = 0.1.  The poisoned token is one every gate of which is open (a question / answer token with a type row and a
# non-zero location), so that the footprint does not hang on what 0 * NaN gives: token row 6 of the text batch, row 3 of the image rows.
# The table sums run in both forms: the fixed-order gather (bits of the clean launch outside F) and the float atomics (rows_scratch =
# NULL), held to the budget the existing tests give the atomic form against the gathered one, 2e-5 * max |clean| + 1e-6.
from test_kernels_gpu import _TEXT_V, _TEXT_NPOS, _TEXT_NTYPES, _IMG_NCOLOR, _text_batch, _text_terms   # noqa: E402


def _atomic_budget(clean):
    return 2e-5 * float(clean.double().abs().max()) + 1e-6


def _kept_column(keep, r):
    """A column of row r that the dropout mask keeps (a dropped NaN is 0: it would poison nothing)."""
    return int(keep[r].nonzero()[-1])


def test_text_embedding_footprint():
    lib = L.load()
    B, T, H, p = 3, 7, 64, 0.1
    M, V, n_pos, n_types = B * T, _TEXT_V, _TEXT_NPOS, _TEXT_NTYPES
    site, seed = 1, (1 << 40) + 0x5EED + B
    ids_c, segs_c, loc_c = _text_batch(B, T, seed=B * 100 + T)
    r = 6
    assert int(segs_c.view(-1)[r]) == -1 and float(loc_c.view(M, 4)[r].abs().sum()) != 0.0      # QA token, type row 0, gate open
    ids, segs = ids_c.to(DEV), segs_c.to(DEV)
    tab = dict(word=rand(V, H, scale=0.5, seed=11), pos=rand(n_pos, H, scale=0.5, seed=12), type=rand(n_types, H, scale=0.5, seed=13),
               w_loc=rand(H, 4, scale=0.5, seed=14), b_loc=rand(H, scale=0.5, seed=15))
    gamma, beta = 1 + 0.1 * rand(H, seed=16), 0.1 * rand(H, seed=17)
    t64 = {k: v.double().cpu() for k, v in tab.items()}
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    thr, sc, st = ops._drop(p, site)
    keep = host_keep(seed, site, M, H, p).cpu()
    stream = L.current_stream()
    loc0 = loc_c.reshape(M, 4).double()

    def fwd(loc):
        locd = _nan_rows(loc, pad=16).float()
        sum_b, y = (torch.full((M + 3, H), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        mean, rstd = torch.full((M + 3,), NAN, device=DEV), torch.full((M + 3,), NAN, device=DEV)
        L.check(lib.crct_embed_text_fwd(ids.data_ptr(), segs.data_ptr(), locd.data_ptr(), tab["word"].data_ptr(), tab["pos"].data_ptr(),
                                        tab["type"].data_ptr(), tab["w_loc"].data_ptr(), tab["b_loc"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        sum_b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, T, H, n_pos, 1e-12, thr, sc, st, seed,
                                        stream), "embed_text_fwd")
        for t in (sum_b, y, mean, rstd):
            assert bool(torch.isnan(t[M:]).all()), "embed_text_fwd wrote behind its last row"
        return dict(sum=sum_b[:M].clone(), y=y[:M].clone(), mean=mean[:M].clone(), rstd=rstd[:M].clone())

    def ref_fwd(loc):
        s = GR.bf16(_text_terms(t64, ids_c, segs_c, loc.view(B, T, 4)))
        mean, _, rstd = _ln_stats64(s)
        yn = g64 * ((s - mean[:, None]) * rstd[:, None]) + b64
        return dict(sum=s, y=torch.where(keep, yn / (1 - p), torch.zeros(())), mean=mean, rstd=rstd)
    clean = fwd(loc0)
    # R4: the clean launch from NaN-padded loc rows against fp64, at the budgets of tests/test_kernels_gpu.py
    t_abs64 = {k: v.abs() for k, v in t64.items()}
    _assert_within_bf16_step(clean["sum"], _text_terms(t64, ids_c, segs_c, loc0.view(B, T, 4)),
                             _text_terms(t_abs64, ids_c, segs_c, loc0.abs().view(B, T, 4)), "embed_text_fwd: clean sum")
    _check_ln_forward(clean["sum"], clean["y"], clean["mean"], clean["rstd"], gamma, beta, p, site, seed, "embed_text_fwd: clean")
    for c, val in ((3, NAN), (0, INF)):
        lp = PR.plant(loc0, (r, c), val)
        F = PR.footprint(ref_fwd, (loc0,), (lp,))
        assert int(F["sum"].sum()) == H and bool(F["sum"][r].all()) and torch.equal(F["y"][r], keep[r]) and int(F["mean"].sum()) == 1
        PR.assert_footprint(clean, fwd(lp), F, "embed_text_fwd, %r in loc(%d, %d)" % (val, r, c))

    # ---- backward from the clean forward's saved state
    sum_b, mean, rstd = clean["sum"], clean["mean"], clean["rstd"]
    dy0 = GR.bf16(rand(M, H, seed=1).cpu())
    names = ("word", "pos", "type", "w_loc", "b_loc", "gamma", "beta")
    shapes = dict(word=(V, H), pos=(n_pos, H), type=(n_types, H), w_loc=(H, 4), b_loc=(H,), gamma=(H,), beta=(H,))
    pre = {k: rand(*s, seed=40 + i) for i, (k, s) in enumerate(shapes.items())}
    index = torch.zeros(2 * V, dtype=torch.int32, device=DEV)
    nblk = lib.crct_layernorm_bwd_blocks(M)
    keep_scale = keep.double() / (1 - p)

    def bwd(dy, loc, mode):
        out = {k: v.clone() for k, v in pre.items()}
        dyd, locd = bf(_nan_rows(dy, pad=16)), _nan_rows(loc, pad=16).float()
        partials = torch.empty(9 * 4 * nblk * H, device=DEV)
        rows = torch.empty(M, H, device=DEV) if mode != "atomic" else None
        idx = torch.empty(2 * M, dtype=torch.int32, device=DEV)
        a = [dyd.data_ptr(), sum_b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ids.data_ptr(), segs.data_ptr(), locd.data_ptr(),
             gamma.data_ptr()] + [out[k].data_ptr() for k in names] + [partials.data_ptr(), B, T, H, n_pos, thr, sc, st, seed, L.ptr(rows),
                                                                       idx.data_ptr(), n_types]
        L.check(lib.crct_embed_text_bwd_indexed(*a, index.data_ptr(), V, stream), "embed_text_bwd " + mode)
        torch.cuda.synchronize()
        return out

    def ref_bwd(dy, loc, mags=False):
        t = {k: v.clone().requires_grad_(True) for k, v in t64.items()}
        ds, dg, db, dg_mag, db_mag = _ln_backward64(sum_b.double().cpu().clone(), dy, keep_scale, gamma)
        grads = torch.autograd.grad(_text_terms(t, ids_c, segs_c, loc.view(B, T, 4)), [t[k] for k in names[:5]], ds)
        out = {k: pre[k].double().cpu() + g for k, g in zip(names, grads)}
        out.update(gamma=pre["gamma"].double().cpu() + dg, beta=pre["beta"].double().cpu() + db)
        if not mags:
            return out
        ta = {k: v.abs().requires_grad_(True) for k, v in t64.items()}     # sum |terms|: the same linear map on |d_sum| with |loc|
        m = torch.autograd.grad(_text_terms(ta, ids_c, segs_c, loc.abs().view(B, T, 4)), [ta[k] for k in names[:5]], ds.abs())
        mag = {k: pre[k].double().cpu().abs() + g for k, g in zip(names, m)}
        mag.update(gamma=pre["gamma"].double().cpu().abs() + dg_mag, beta=pre["beta"].double().cpu().abs() + db_mag)
        return out, mag
    c = _kept_column(keep, r)
    # ... and a token whose location gate is CLOSED (row 0: a QA token with an all-zero loc).  The reference multiplies by the gate, so the
    # NaN row gradient reaches d W_loc and d b_loc through NaN * 0: the kernel's gate is a factor too, not a skipped row.
    r0 = 0
    assert int(segs_c.view(-1)[r0]) == 1 and float(loc0[r0].abs().sum()) == 0.0
    c0 = _kept_column(keep, r0)
    cases = (("NaN in dy(%d, %d)" % (r, c), (PR.plant(dy0, (r, c), NAN), loc0)), ("inf in loc(%d, 1)" % r, (dy0, PR.plant(loc0, (r, 1), INF))),
             ("NaN in dy(%d, %d), gate closed" % (r0, c0), (PR.plant(dy0, (r0, c0), NAN), loc0)))
    ref_c, mag_c = ref_bwd(dy0, loc0, mags=True)
    for mode in ("indexed", "atomic"):
        clean_b = bwd(dy0, loc0, mode)
        for k in names:
            _assert_sums(clean_b[k], ref_c[k], mag_c[k], "embed_text_bwd (%s): clean d_%s" % (mode, k))
        budgets = {k: (_atomic_budget(clean_b[k]) if mode == "atomic" and k in ("word", "pos", "type") else False) for k in names}
        for what, pois in cases:
            F = PR.footprint(ref_bwd, (dy0, loc0), pois)
            if what.startswith("NaN"):         # the token's table rows, every word of the location Linear, column c of the LayerNorm's
                rr = r0 if what.endswith("closed") else r
                assert int(F["word"].sum()) == H and bool(F["word"][int(ids_c.view(-1)[rr])].all()) and int(F["type"].sum()) == H
                assert int(F["pos"].sum()) == H and bool(F["w_loc"].all()) and bool(F["b_loc"].all()) and int(F["gamma"].sum()) == 1
            else:                              # loc is a factor of d W_loc alone: its column 1
                assert {k: int(v.sum()) for k, v in F.items()} == dict(word=0, pos=0, type=0, w_loc=H, b_loc=0, gamma=0, beta=0)
            PR.assert_footprint(clean_b, bwd(*pois, mode), F, "embed_text_bwd (%s), %s" % (mode, what), atomic=budgets)


def test_image_embedding_footprint():
    lib = L.load()
    M, H, p = 7, 64, 0.1
    n_color, site, seed = _IMG_NCOLOR, 2, (3 << 60) + 0xC0FFEE + M
    g = torch.Generator().manual_seed(M + H)
    target = torch.randint(0, n_color, (M,), generator=g)
    target[: M // 3] = 17
    target[-1] = 0
    loc0 = (torch.rand(M, 4, generator=g) + 0.1).double()
    img0 = GR.bf16(rand(M, H, scale=0.5, seed=21).cpu())
    tab = dict(color=rand(n_color, H, scale=0.5, seed=22), w_loc=rand(H, 4, scale=0.5, seed=23), b_loc=rand(H, scale=0.5, seed=24))
    gamma, beta = 1 + 0.1 * rand(H, seed=25), 0.1 * rand(H, seed=26)
    t64 = {k: v.double().cpu() for k, v in tab.items()}
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    target_d = target.to(DEV)
    thr, sc, st = ops._drop(p, site)
    keep = host_keep(seed, site, M, H, p).cpu()
    keep_scale = keep.double() / (1 - p)
    stream = L.current_stream()
    r = 3

    def fwd(img, loc):
        imgd, locd = bf(_nan_rows(img, pad=16)), _nan_rows(loc, pad=16).float()
        sum_b, y = (torch.full((M + 3, H), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        mean, rstd = torch.full((M + 3,), NAN, device=DEV), torch.full((M + 3,), NAN, device=DEV)
        L.check(lib.crct_embed_image_fwd(imgd.data_ptr(), locd.data_ptr(), target_d.data_ptr(), tab["w_loc"].data_ptr(), tab["b_loc"].data_ptr(),
                                         tab["color"].data_ptr(), gamma.data_ptr(), beta.data_ptr(), sum_b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), M, H, 1e-12, thr, sc, st, seed, stream), "embed_image_fwd")
        for t in (sum_b, y, mean, rstd):
            assert bool(torch.isnan(t[M:]).all()), "embed_image_fwd wrote behind its last row"
        return dict(sum=sum_b[:M].clone(), y=y[:M].clone(), mean=mean[:M].clone(), rstd=rstd[:M].clone())

    def terms(t, img, loc):
        return img + loc @ t["w_loc"].t() + t["b_loc"] + t["color"][target]

    def ref_fwd(img, loc):
        s = GR.bf16(terms(t64, img, loc))
        mean, _, rstd = _ln_stats64(s)
        yn = g64 * ((s - mean[:, None]) * rstd[:, None]) + b64
        return dict(sum=s, y=torch.where(keep, yn / (1 - p), torch.zeros(())), mean=mean, rstd=rstd)
    clean = fwd(img0, loc0)
    t_abs64 = {k: v.abs() for k, v in t64.items()}
    _assert_within_bf16_step(clean["sum"], terms(t64, img0, loc0), terms(t_abs64, img0.abs(), loc0.abs()), "embed_image_fwd: clean sum")
    _check_ln_forward(clean["sum"], clean["y"], clean["mean"], clean["rstd"], gamma, beta, p, site, seed, "embed_image_fwd: clean")
    for what, pois in (("NaN image feature", (PR.plant(img0, (r, H - 1), NAN), loc0)), ("inf loc", (img0, PR.plant(loc0, (r, 0), INF)))):
        F = PR.footprint(ref_fwd, (img0, loc0), pois)
        # the feature is an addend of its own element of the sum; the location Linear spreads an inf over the row; LayerNorm spreads both
        assert int(F["sum"].sum()) == (1 if what.startswith("NaN") else H) and bool(F["sum"][r].any()) and not bool(F["sum"][:r].any())
        assert torch.equal(F["y"][r], keep[r]) and int(F["y"].sum()) == int(keep[r].sum()) and int(F["rstd"].sum()) == 1 and bool(F["mean"][r])
        PR.assert_footprint(clean, fwd(*pois), F, "embed_image_fwd, " + what)

    sum_b, mean, rstd = clean["sum"], clean["mean"], clean["rstd"]
    dy0 = GR.bf16(rand(M, H, seed=2).cpu())
    names = ("color", "w_loc", "b_loc", "b_img", "gamma", "beta")
    shapes = dict(color=(n_color, H), w_loc=(H, 4), b_loc=(H,), b_img=(H,), gamma=(H,), beta=(H,))
    pre = {k: rand(*s, seed=60 + i) for i, (k, s) in enumerate(shapes.items())}
    nblk = lib.crct_layernorm_bwd_blocks(M)

    def bwd(dy, loc, mode):
        out = {k: v.clone() for k, v in pre.items()}
        dyd, locd = bf(_nan_rows(dy, pad=16)), _nan_rows(loc, pad=16).float()
        d_sum = torch.full((M + 3, H), NAN, device=DEV, dtype=torch.bfloat16)
        partials = torch.empty(7 * 4 * nblk * H, device=DEV)
        rows = torch.empty(M, H, device=DEV) if mode == "gather" else None
        idx = torch.empty(M, dtype=torch.int32, device=DEV)
        L.check(lib.crct_embed_image_bwd(dyd.data_ptr(), sum_b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), locd.data_ptr(), target_d.data_ptr(),
                                         gamma.data_ptr(), d_sum.data_ptr(), out["color"].data_ptr(), out["w_loc"].data_ptr(), out["b_loc"].data_ptr(),
                                         out["b_img"].data_ptr(), out["gamma"].data_ptr(), out["beta"].data_ptr(), partials.data_ptr(), M, H,
                                         thr, sc, st, seed, L.ptr(rows), idx.data_ptr(), n_color, stream), "embed_image_bwd " + mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_sum[M:]).all()), "embed_image_bwd wrote behind the last row of d_sum"
        return dict(out, d_sum=d_sum[:M].clone())

    def ref_bwd(dy, loc, mags=False):
        t = {k: v.clone().requires_grad_(True) for k, v in t64.items()}
        ds, dg, db, dg_mag, db_mag = _ln_backward64(sum_b.double().cpu().clone(), dy, keep_scale, gamma)
        grads = torch.autograd.grad(terms(t, img0, loc), [t[k] for k in names[:3]], ds)
        out = {k: pre[k].double().cpu() + g for k, g in zip(names, grads)}
        out.update(b_img=pre["b_img"].double().cpu() + ds.sum(0), gamma=pre["gamma"].double().cpu() + dg, beta=pre["beta"].double().cpu() + db, d_sum=ds)
        if not mags:
            return out
        ta = {k: v.abs().requires_grad_(True) for k, v in t64.items()}
        m = torch.autograd.grad(terms(ta, img0.abs(), loc.abs()), [ta[k] for k in names[:3]], ds.abs())
        mag = {k: pre[k].double().cpu().abs() + g for k, g in zip(names, m)}
        mag.update(b_img=pre["b_img"].double().cpu().abs() + ds.abs().sum(0), gamma=pre["gamma"].double().cpu().abs() + dg_mag,
                   beta=pre["beta"].double().cpu().abs() + db_mag)
        return out, mag
    ref_c, mag_c = ref_bwd(dy0, loc0, mags=True)
    c = _kept_column(keep, r)
    cases = (("NaN in dy(%d, %d)" % (r, c), (PR.plant(dy0, (r, c), NAN), loc0)), ("inf in loc(%d, 2)" % r, (dy0, PR.plant(loc0, (r, 2), INF))))
    for mode in ("gather", "atomic"):
        clean_b = bwd(dy0, loc0, mode)
        for k in names:
            _assert_sums(clean_b[k], ref_c[k], mag_c[k], "embed_image_bwd (%s): clean d_%s" % (mode, k))
        budgets = {k: (_atomic_budget(clean_b[k]) if mode == "atomic" and k == "color" else False) for k in list(names) + ["d_sum"]}
        for what, pois in cases:
            F = PR.footprint(ref_bwd, (dy0, loc0), pois)
            if what.startswith("NaN"):
                assert int(F["d_sum"].sum()) == H and bool(F["d_sum"][r].all()) and int(F["color"].sum()) == H and bool(F["color"][int(target[r])].all())
                assert bool(F["w_loc"].all()) and bool(F["b_loc"].all()) and bool(F["b_img"].all()) and int(F["gamma"].sum()) == 1
            else:
                assert {k: int(v.sum()) for k, v in F.items()} == dict(color=0, w_loc=H, b_loc=0, b_img=0, gamma=0, beta=0, d_sum=0)
            PR.assert_footprint(clean_b, bwd(*pois, mode), F, "embed_image_bwd (%s), %s" % (mode, what), atomic=budgets)


def test_embed_input_grad_footprint():
    """crct_embed_input_grad (d_loc, d_areas, d_sum from an embedding's saved LayerNorm state): a NaN in dy(r, c) or in the saved sum's
    row r stays in row r of the three outputs."""
    M, H, p, site, seed = 7, 64, 0.1, 2, (3 << 60) + 0xC0FFEE
    x0 = GR.bf16((rand(M, H, scale=2.0, seed=3) + 0.3).cpu())
    dy0 = GR.bf16(rand(M, H, seed=4).cpu())
    gamma = 1 + 0.1 * rand(H, seed=5)
    w_loc, w_areas = rand(H, 4, scale=0.5, seed=6), rand(H, scale=0.5, seed=7)
    loc = (torch.rand(M, 4, generator=torch.Generator().manual_seed(8)) + 0.1).to(DEV)
    keep = host_keep(seed, site, M, H, p).cpu()
    keep_scale = keep.double() / (1 - p)
    r = 4

    def run(dy, x):
        xb = bf(_nan_rows(x, pad=16))[:M]
        _, mean, rstd = ops.layernorm_fwd(xb, gamma, torch.zeros_like(gamma))
        d_loc, d_areas, d_sum = ops.embed_input_grad(bf(_nan_rows(dy, pad=16))[:M], xb, mean, rstd, gamma, loc=loc, w_loc=w_loc, w_areas=w_areas,
                                                     p_drop=p, site=site, seed=seed)
        return dict(d_loc=d_loc, d_areas=d_areas, d_sum=d_sum)

    def ref(dy, x):
        ds = _ln_backward64(x.detach().clone(), dy, keep_scale, gamma)[0]
        return dict(d_loc=ds @ w_loc.double().cpu(), d_areas=ds @ w_areas.double().cpu(), d_sum=ds)
    clean = run(dy0, x0)
    _, mean_c, rstd_c = ops.layernorm_fwd(bf(x0.to(DEV)), gamma, torch.zeros_like(gamma))
    args = (bf(dy0), bf(x0), mean_c.cpu(), rstd_c.cpu(), gamma.cpu(), keep, p, w_loc.cpu(), loc.cpu(), w_areas.cpu())
    ref_c, bud_c = IG.rows_reference(*args), IG.rows_budget(*args)
    for k in ("d_loc", "d_areas", "d_sum"):
        ratio = IG.ratio(clean[k], ref_c[k], bud_c[k])
        assert float(ratio.max()) <= 1.0, ("embed_input_grad: clean " + k, float(ratio.max()))
    c = _kept_column(keep, r)
    for what, pois in (("NaN in dy", (PR.plant(dy0, (r, c), NAN), x0)), ("NaN in the saved sum", (dy0, PR.plant(x0, (r, 0), NAN)))):
        F = PR.footprint(ref, (dy0, x0), pois)
        assert {k: int(v.sum()) for k, v in F.items()} == dict(d_loc=4, d_areas=1, d_sum=H) and bool(F["d_sum"][r].all())
        PR.assert_footprint(clean, run(*pois), F, "embed_input_grad, " + what)


def test_image_variant_embedding_with_areas_footprint():
    """crct_embed_image_var_fwd / _bwd (dvqa / figure_qa: no feature term, areas_emp(areas) when areas are given), M = 7, H = 64, p = 0.1.
    A NaN in areas[r] poisons row r of the sum, the kept elements of y and mean / rstd; in the backward (from the clean saved state) it
    reaches d W_areas alone.  A NaN in dy(r, c) reaches the colour row of target[r], every word of both Linears' gradients and column c of
    the LayerNorm's.  areas carries NaN behind its last row; the launch WITHOUT areas (areas = NULL is the flag) is handed NaN-filled
    w_areas / b_areas and must give the bits of the launch with finite ones, its d W_areas / d b_areas untouched."""
    lib = L.load()
    M, H, p, n_color = 7, 64, 0.1, 11
    site, seed = 2, (3 << 60) + 0xA4EA5
    g = torch.Generator().manual_seed(M * H)
    target = torch.randint(0, n_color, (M,), generator=g)
    target[:2] = 5
    loc0 = (torch.rand(M, 4, generator=g) + 0.1).double()
    areas0 = (torch.rand(M, generator=g) + 0.1).double()
    tab = dict(color=rand(n_color, H, scale=0.5, seed=22), w_loc=rand(H, 4, scale=0.5, seed=23), b_loc=rand(H, scale=0.5, seed=24),
               w_areas=rand(H, 1, scale=0.5, seed=25), b_areas=rand(H, scale=0.5, seed=26))
    gamma, beta = 1 + 0.1 * rand(H, seed=27), 0.1 * rand(H, seed=28)
    t64 = {k: v.double().cpu() for k, v in tab.items()}
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    target_d = target.to(DEV)
    thr, sc, st = ops._drop(p, site)
    keep = host_keep(seed, site, M, H, p).cpu()
    keep_scale = keep.double() / (1 - p)
    stream = L.current_stream()
    nanvec = {k: torch.full_like(tab[k], NAN) for k in ("w_areas", "b_areas")}
    r = 4

    def terms(t, loc, areas):
        e = loc @ t["w_loc"].t() + t["b_loc"] + t["color"][target]
        return e if areas is None else e + areas[:, None] * t["w_areas"][:, 0] + t["b_areas"]

    def fwd(loc, areas, wa=None, ba=None):
        locd = _nan_rows(loc, pad=16).float()
        ard = None if areas is None else torch.cat([areas, torch.full((16,), NAN, dtype=torch.float64)]).float().to(DEV)
        wa, ba = tab["w_areas"] if wa is None else wa, tab["b_areas"] if ba is None else ba
        sum_b, y = (torch.full((M + 3, H), NAN, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        mean, rstd = torch.full((M + 3,), NAN, device=DEV), torch.full((M + 3,), NAN, device=DEV)
        L.check(lib.crct_embed_image_var_fwd(locd.data_ptr(), target_d.data_ptr(), L.ptr(ard), tab["w_loc"].data_ptr(), tab["b_loc"].data_ptr(),
                                             tab["color"].data_ptr(), wa.data_ptr(), ba.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             sum_b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, H, 1e-12, thr, sc, st, seed,
                                             stream), "embed_image_var_fwd")
        for t in (sum_b, y, mean, rstd):
            assert bool(torch.isnan(t[M:]).all()), "embed_image_var_fwd wrote behind its last row"
        return dict(sum=sum_b[:M].clone(), y=y[:M].clone(), mean=mean[:M].clone(), rstd=rstd[:M].clone())

    def ref_fwd(loc, areas):
        s = GR.bf16(terms(t64, loc, areas))
        mean, _, rstd = _ln_stats64(s)
        yn = g64 * ((s - mean[:, None]) * rstd[:, None]) + b64
        return dict(sum=s, y=torch.where(keep, yn / (1 - p), torch.zeros(())), mean=mean, rstd=rstd)
    clean = fwd(loc0, areas0)
    t_abs64 = {k: v.abs() for k, v in t64.items()}
    _assert_within_bf16_step(clean["sum"], terms(t64, loc0, areas0), terms(t_abs64, loc0.abs(), areas0.abs()), "embed_image_var_fwd: clean sum")
    _check_ln_forward(clean["sum"], clean["y"], clean["mean"], clean["rstd"], gamma, beta, p, site, seed, "embed_image_var_fwd: clean")
    for what, pois in (("NaN in areas", (loc0, PR.plant(areas0, r, NAN))), ("inf in loc", (PR.plant(loc0, (r, 3), INF), areas0))):
        F = PR.footprint(ref_fwd, (loc0, areas0), pois)
        assert int(F["sum"].sum()) == H and bool(F["sum"][r].all()) and torch.equal(F["y"][r], keep[r]) and int(F["mean"].sum()) == 1
        PR.assert_footprint(clean, fwd(*pois), F, "embed_image_var_fwd, " + what)
    # the launch without areas: NaN-filled w_areas / b_areas are ignored memory
    plain = fwd(loc0, None)
    _assert_within_bf16_step(plain["sum"], terms(t64, loc0, None), terms(t_abs64, loc0.abs(), None), "embed_image_var_fwd without areas: sum")
    ignored = fwd(loc0, None, wa=nanvec["w_areas"], ba=nanvec["b_areas"])
    for k in plain:
        assert torch.equal(PR.bits(ignored[k]), PR.bits(plain[k])), "embed_image_var_fwd without areas reads w_areas / b_areas: " + k

    sum_b, mean, rstd = clean["sum"], clean["mean"], clean["rstd"]
    dy0 = GR.bf16(rand(M, H, seed=2).cpu())
    names = ("color", "w_loc", "b_loc", "w_areas", "b_areas", "gamma", "beta")
    pre = {k: rand(*(tab[k].shape if k in tab else (H,)), seed=60 + i) for i, k in enumerate(names)}
    nblk = lib.crct_layernorm_bwd_blocks(M)

    def bwd(dy, loc, areas, mode, saved=None):
        sb, mn, rs = saved or (sum_b, mean, rstd)
        out = {k: v.clone() for k, v in pre.items()}
        dyd, locd = bf(_nan_rows(dy, pad=16)), _nan_rows(loc, pad=16).float()
        ard = None if areas is None else torch.cat([areas, torch.full((16,), NAN, dtype=torch.float64)]).float().to(DEV)
        partials = torch.empty(8 * 4 * nblk * H, device=DEV)
        rows = torch.empty(M, H, device=DEV) if mode == "gather" else None
        idx = torch.empty(M, dtype=torch.int32, device=DEV)
        L.check(lib.crct_embed_image_var_bwd(dyd.data_ptr(), sb.data_ptr(), mn.data_ptr(), rs.data_ptr(), locd.data_ptr(), target_d.data_ptr(),
                                             L.ptr(ard), gamma.data_ptr(), *[out[k].data_ptr() for k in names], partials.data_ptr(), M, H,
                                             thr, sc, st, seed, L.ptr(rows), idx.data_ptr(), n_color, stream), "embed_image_var_bwd " + mode)
        torch.cuda.synchronize()
        return out

    def ref_bwd(dy, loc, areas, mags=False):
        t = {k: v.clone().requires_grad_(True) for k, v in t64.items()}
        ds, dg, db, dg_mag, db_mag = _ln_backward64(sum_b.double().cpu().clone(), dy, keep_scale, gamma)
        grads = torch.autograd.grad(terms(t, loc, areas), [t[k] for k in names[:5]], ds)
        out = {k: pre[k].double().cpu() + g for k, g in zip(names, grads)}
        out.update(gamma=pre["gamma"].double().cpu() + dg, beta=pre["beta"].double().cpu() + db)
        if not mags:
            return out
        ta = {k: v.abs().requires_grad_(True) for k, v in t64.items()}
        m = torch.autograd.grad(terms(ta, loc.abs(), areas.abs()), [ta[k] for k in names[:5]], ds.abs())
        mag = {k: pre[k].double().cpu().abs() + g for k, g in zip(names, m)}
        mag.update(gamma=pre["gamma"].double().cpu().abs() + dg_mag, beta=pre["beta"].double().cpu().abs() + db_mag)
        return out, mag
    ref_c, mag_c = ref_bwd(dy0, loc0, areas0, mags=True)
    c = _kept_column(keep, r)
    cases = (("NaN in areas(%d)" % r, (dy0, loc0, PR.plant(areas0, r, NAN))), ("NaN in dy(%d, %d)" % (r, c), (PR.plant(dy0, (r, c), NAN), loc0, areas0)))
    for mode in ("gather", "atomic"):
        clean_b = bwd(dy0, loc0, areas0, mode)
        for k in names:
            _assert_sums(clean_b[k], ref_c[k], mag_c[k], "embed_image_var_bwd (%s): clean d_%s" % (mode, k))
        budgets = {k: (_atomic_budget(clean_b[k]) if mode == "atomic" and k == "color" else False) for k in names}
        for what, pois in cases:
            F = PR.footprint(ref_bwd, (dy0, loc0, areas0), pois)
            if "areas" in what:                # areas is a factor of d W_areas alone
                assert {k: int(v.sum()) for k, v in F.items()} == dict(color=0, w_loc=0, b_loc=0, w_areas=H, b_areas=0, gamma=0, beta=0)
            else:
                assert int(F["color"].sum()) == H and bool(F["color"][int(target[r])].all()) and int(F["gamma"].sum()) == 1
                assert all(bool(F[k].all()) for k in ("w_loc", "b_loc", "w_areas", "b_areas"))
            # d W_areas [H, 1] depends on areas[r] in every element: R3's proper footprint is taken over the areas Linear's gradient as a
            # whole (weight and bias side by side), where the NaN must be in the weight half and nowhere in the bias half
            def whole(o):
                return dict(o, areas_emp=torch.cat([o["w_areas"].reshape(-1), o["b_areas"].reshape(-1)]))
            PR.assert_footprint(whole(clean_b), whole(bwd(*pois, mode)), whole(F), "embed_image_var_bwd (%s), %s" % (mode, what),
                                atomic=dict(budgets, areas_emp=False))
    # without areas, from that launch's own saved state: d W_areas / d b_areas keep the prefilled bits, the rest does not depend on them
    saved = (plain["sum"], plain["mean"], plain["rstd"])
    off = bwd(dy0, loc0, None, "gather", saved=saved)
    for k in ("w_areas", "b_areas"):
        assert torch.equal(PR.bits(off[k]), PR.bits(pre[k])), "embed_image_var_bwd without areas wrote d_" + k
    assert all(bool(torch.isfinite(off[k]).all()) for k in names)
