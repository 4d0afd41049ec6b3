"""Head size 128 (the original ViLBERT config's visual stream and co-attention) in every attention entry point, per element against fp64
(-m gpu).  The method is tests/test_attention_gpu.py's, with own copies of its small helpers: q, k, v are column slices of fused
[*, 3 H + 8] buffers, the outputs go into slices of sentinel-filled canvases with guard rows, every element is compared with the fp64
reference of tests/attention_ref.py under its derived budget (tests/test_attention_head128_cpu.py proves the yardstick at d = 128), the
dropout mask is the host Philox copy's (tests/dropout_ref.py).

d = 128 runs on csrc/attention_long.hip's blocked kernels (attn_fwd_blk / attn_bwd_blk: image blocks of 256 rows) at EVERY length; the
lengths below reach one and two blocks per side, a length exactly at the block boundary (256) and one tile past it (272, 257 with a
ragged tile), 4 and 8 waves, kept and recomputed statistics, the dropout-bit cache on and off.

Largest |got - fp64| / (bf16 step + budget) measured on the MI355X (each test prints its own; run with -s): lengths up to 112 0.83 (ctx,
4 query tiles), the long cases 0.79 (dq, 36 x 36 forced; 0.72 at 512 x 512), the maps 0.50 (512 x 300) -- the emulator's figures
(tests/test_attention_head128_cpu.py: 0.79) to two digits.
"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import attention_ref as AR        # noqa: E402
import attention_probs_ref as PR  # noqa: E402
import dropout_ref as DR          # noqa: E402

DEV = "cuda"
D = 128
SEED, SITE = 20240917, 11
SENTINEL = 0x7B7B                 # bf16 bit pattern (1.3e36) no attention output takes
SENTINEL32 = 0x7B7B7B7B           # fp32 bit pattern no probability takes
GUARD_ROWS = 3
GUARD = 67


@contextlib.contextmanager
def _hooks(valu=0, long=0, split=0):
    lib = L.load()
    try:
        lib.crct_attention_force_valu(valu)
        lib.crct_attention_force_long(long)
        lib.crct_attention_force_split(split)
        yield
    finally:
        lib.crct_attention_force_valu(0)
        lib.crct_attention_force_long(0)
        lib.crct_attention_force_split(0)


class _Canvas:
    """[B, T, ld] bf16 rows + GUARD_ROWS guard rows, all SENTINEL; view(c0, H) is the [B, T, H] column slice a kernel writes."""

    def __init__(self, B, T, ld):
        self.B, self.T, self.ld = B, T, ld
        self.raw = torch.full(((B * T + GUARD_ROWS) * ld,), SENTINEL, dtype=torch.int16, device=DEV)
        self.written = torch.zeros((B * T + GUARD_ROWS) * ld, dtype=torch.bool)

    def view(self, c0, H):
        self.written[:self.B * self.T * self.ld].view(self.B, self.T, self.ld)[:, :, c0:c0 + H] = True
        return self.raw.view(torch.bfloat16)[:self.B * self.T * self.ld].view(self.B, self.T, self.ld)[:, :, c0:c0 + H]

    def assert_intact(self, what):
        raw = self.raw.cpu()
        touched = (raw != SENTINEL) & ~self.written
        assert not bool(touched.any()), "%s: %d elements outside the output slices overwritten, first at flat index %d (ld %d)" % (
            what, int(touched.sum()), int(touched.nonzero()[0]), self.ld)
        assert not bool((raw[self.written] == SENTINEL).any()), "%s: output elements never written" % what


class _Case:
    """Operands of one case on the device (as slices of fused buffers) with the keep mask; the fp64 reference is made once per form."""

    def __init__(self, family, B, heads, Tq, Tk, p, idx, d=D):
        self.B, self.heads, self.Tq, self.Tk, self.d, self.p = B, heads, Tq, Tk, d, p
        self.what = "%s B=%d heads=%d %dx%dx%d p=%g" % (family, B, heads, Tq, Tk, d, p)
        H = self.H = heads * d
        self.q, self.k, self.v, self.dctx, self.km = AR.make_inputs(family, B, heads, Tq, Tk, d, seed=idx, mask_offset=idx)
        g = torch.Generator().manual_seed(idx)
        bufq = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g))        # the neighbours hold data, not zeros
        bufk = AR.bf16(torch.randn(B, Tk, 3 * H + 8, generator=g))
        bufo = AR.bf16(torch.randn(B, Tq, H + 8, generator=g))
        bufq[:, :, :H], bufk[:, :, H:2 * H], bufk[:, :, 2 * H:3 * H], bufo[:, :, 8:] = self.q, self.k, self.v, self.dctx
        bufq, bufk, bufo = bufq.to(DEV), bufk.to(DEV), bufo.to(DEV)
        self.q_, self.k_, self.v_, self.do_ = bufq[:, :, :H], bufk[:, :, H:2 * H], bufk[:, :, 2 * H:3 * H], bufo[:, :, 8:]
        self.km_ = self.km.to(DEV)
        self.keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
        self._ref = {}

    def ref(self, ctx_bf16=None):
        key = None if ctx_bf16 is None else "kept"
        if key not in self._ref:
            self._ref[key] = AR.reference(self.q, self.k, self.v, self.km, self.dctx, self.heads, self.d, keep=self.keep, p=self.p, ctx_bf16=ctx_bf16)
        return self._ref[key]

    def launch(self, kept=False):
        """Forward and backward into fresh sentinel canvases -> (outputs on the host, lse, canvases)."""
        B, heads, Tq, Tk, d, H, p = self.B, self.heads, self.Tq, self.Tk, self.d, self.H, self.p
        c_ctx, c_dq, c_dkv = _Canvas(B, Tq, H + 8), _Canvas(B, Tq, 3 * H), _Canvas(B, Tk, 3 * H)
        ctx, dq, dk, dv = c_ctx.view(0, H), c_dq.view(0, H), c_dkv.view(H, H), c_dkv.view(2 * H, H)
        lse = torch.full((B, heads, Tq), float("nan"), device=DEV) if kept else None
        out = ops.attention_fwd(self.q_, self.k_, self.v_, self.km_, heads, d, p_drop=p, site=SITE, seed=SEED, row_lse=lse, out=ctx)
        assert out.data_ptr() == ctx.data_ptr()
        ops.attention_bwd(self.q_, self.k_, self.v_, self.km_, self.do_, heads, d, p_drop=p, site=SITE, seed=SEED, row_lse=lse,
                          ctx=ctx if kept else None, outs=(dq, dk, dv))
        torch.cuda.synchronize()
        return dict(ctx=ctx.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu()), lse, (c_ctx, c_dq, c_dkv)

    def run(self, tag, kept=False, worst=None):
        """launch() + per-element budget, intact sentinels, and (kept) row_lse against fp64.  Returns the outputs."""
        what = "%s [%s%s]" % (self.what, tag, ", kept statistics" if kept else "")
        got, lse, canvases = self.launch(kept)
        ref = self.ref(got["ctx"] if kept else None)
        for n in AR.OUTPUTS:
            x = AR.assert_within(got[n], ref[n], AR.budget_of(ref, n, kept), "%s: %s" % (what, n))
            if worst is not None:
                worst[n] = max(worst.get(n, 0.0), x)
        for c, n in zip(canvases, ("ctx", "dq", "dk / dv")):
            c.assert_intact("%s: %s canvas" % (what, n))
        if kept:
            err = (lse.double().cpu() - ref["lse"]).abs()       # log2 sum_j exp2(x_ij) against fp64, within fp32 slack at that magnitude
            bad = err > 2.0 ** -16 * (1.0 + ref["lse"].abs())
            assert not bool(bad.any()), "%s: row_lse: %d rows off, first at %s" % (what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]))
        return got


def _show(title, worst, n_cases):
    print("%s: %d runs, largest |got - fp64| / budget: " % (title, n_cases) + ", ".join("%s %.2f" % (n, worst.get(n, 0.0)) for n in AR.OUTPUTS))


# ------------------------------------------------------------------------------------------- lengths up to 112
SHORT = (5, 17, 36, 49)
SEVEN = (65, 81, 112)
SPLITS = (0, 1, 2, 4)             # crct_attention_force_split: every count the library knows


def _sweep_lengths(iq):
    """The five (Tq, Tk) of query-tile class iq of {1, 2, 3, 4, 7}^2 with their case index (tests/test_attention_gpu.py _sweep_lengths)."""
    out = []
    for ik in range(5):
        Tq = SHORT[iq] if iq < 4 else SEVEN[(iq + 2 * ik) % 3]
        Tk = SHORT[ik] if ik < 4 else SEVEN[(2 * iq + ik + 1) % 3]
        out.append((5 * iq + ik, Tq, Tk))
    return out


def test_the_sweep_covers_every_tile_pair_and_all_seven_lengths():
    lens = [c for iq in range(5) for c in _sweep_lengths(iq)]
    tiles = lambda T: 7 if (T + 15) // 16 > 4 else (T + 15) // 16      # noqa: E731
    assert len({(tiles(Tq), tiles(Tk)) for _, Tq, Tk in lens}) == 25
    assert {T for _, Tq, Tk in lens for T in (Tq, Tk)} == set(SHORT + SEVEN)


@pytest.mark.parametrize("iq", range(5))
def test_every_tile_pair_up_to_112_against_fp64_and_the_same_bits_for_every_split(iq):
    """All 25 pairs of the tile counts {1, 2, 3, 4, 7}^2 (five per case of this test) at d = 128, B = 2, heads = 2, p = 0.1, the diagonal
    once more with p = 0; under every crct_attention_force_split count the outputs are bit-identical."""
    worst, n = {}, 0
    for idx, Tq, Tk in _sweep_lengths(iq):
        for p in ((0.1, 0.0) if idx % 6 == 0 else (0.1,)):            # idx = 6 iq on the diagonal
            case = _Case(AR.FAMILIES[idx % 5], 2, 2, Tq, Tk, p, idx)
            first = None
            for split in SPLITS:
                with _hooks(split=split):
                    if first is None:
                        first = case.run("force_split %d" % split, worst=worst)
                    else:
                        got, _, _ = case.launch()
                        for name in AR.OUTPUTS:
                            assert torch.equal(got[name], first[name]), "%s: %s differs between force_split %d and %d" % (case.what, name, SPLITS[0], split)
                n += 1
    _show("d=128 up to 112, query class %d" % iq, worst, n)


# ------------------------------------------------------------------------------------------- long kernels
# (Tq, Tk, B, heads, force_long)
LONG_CASES = [
    (113, 5, 2, 1, 0), (5, 113, 2, 1, 0), (124, 44, 2, 2, 0), (44, 124, 2, 2, 0), (130, 130, 1, 2, 0), (257, 40, 1, 2, 0), (40, 257, 1, 2, 0),
    (256, 256, 1, 2, 0),          # exactly one block of 16 tiles per side
    (272, 300, 1, 2, 0),          # one tile past the block boundary
    (511, 512, 1, 1, 0), (512, 512, 1, 2, 0),
    (36, 36, 2, 2, 1), (112, 65, 2, 2, 1),      # force_long: the same kernels (d = 128 has no other), held to the short shapes under the hook too
]


@pytest.mark.parametrize("idx", range(len(LONG_CASES)), ids=["%dx%d%s" % (a, b, "-forced" if f else "") for a, b, _, _, f in LONG_CASES])
def test_long_kernels_at_head_size_128_against_fp64(idx):
    """LONG_CASES[idx]: p in {0, 0.1} x {recomputed, kept} statistics; with kept statistics also row_lse per element against fp64."""
    Tq, Tk, B, heads, force = LONG_CASES[idx]
    worst, n = {}, 0
    for ip, p in enumerate((0.0, 0.1)):
        case = _Case(AR.FAMILIES[(idx + ip) % 5], B, heads, Tq, Tk, p, 100 + 2 * idx + ip)
        for kept in (False, True):
            with _hooks(long=force):
                case.run("long", kept=kept, worst=worst)
            n += 1
    _show("d=128 long %dx%d%s" % (Tq, Tk, " (forced)" if force else ""), worst, n)


def test_force_valu_leaves_head_size_128_on_the_mfma_kernels():
    case = _Case("flat", 2, 2, 36, 49, 0.1, 7)
    plain, _, _ = case.launch()
    with _hooks(valu=1):
        forced = case.run("force_valu")
    for name in AR.OUTPUTS:
        assert torch.equal(plain[name], forced[name]), name


@pytest.mark.parametrize("Tq,Tk", [(44, 124), (112, 112), (300, 512)])
def test_forward_and_backward_twice_give_the_same_bits(Tq, Tk):
    case = _Case("flat", 2, 2, Tq, Tk, 0.1, 300 + Tq)
    for kept in (False, True):
        a, lse_a, _ = case.launch(kept)
        b, lse_b, _ = case.launch(kept)
        for name in AR.OUTPUTS:
            assert torch.equal(a[name], b[name]), (name, kept)
        if kept:
            assert torch.equal(lse_a, lse_b)


# ------------------------------------------------------------------------------------------- dropout masks
@pytest.mark.parametrize("Tq,Tk", [(36, 36), (124, 44)])
def test_the_dropout_mask_does_not_depend_on_the_head_size(Tq, Tk):
    """Equal (seed, site, B heads, Tq, Tk): the keep pattern read off the maps (zero / non-zero; every key attended, small scores, so no
    probability underflows) is the same at d = 64 and d = 128, and is tests/dropout_ref.py's."""
    B, heads, p = 2, 2, 0.1
    want = torch.as_tensor(DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p)).reshape(B, heads, Tq, Tk).bool()
    assert 0.8 < float(want.float().mean()) < 0.97
    pats = {}
    for d in (64, 128):
        g = torch.Generator().manual_seed(d)
        q = (torch.randn(B, Tq, heads * d, generator=g) * 0.1).bfloat16().to(DEV)
        k = (torch.randn(B, Tk, heads * d, generator=g) * 0.1).bfloat16().to(DEV)
        km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
        pats[d] = (ops.attention_probs(q, k, km, heads, d, p_drop=p, site=SITE, seed=SEED) != 0).cpu()
    assert torch.equal(pats[64], pats[128])
    assert torch.equal(pats[128], want)


# ------------------------------------------------------------------------------------------- maps
def _run_probs(family, B, heads, Tq, Tk, p, idx):
    """One case of ops.attention_probs at d = 128 at every output offset that takes another store path (tests/test_attention_probs_gpu.py
    _run).  Returns the largest budget ratio."""
    what = "%s B=%d heads=%d %dx%dx%d p=%g" % (family, B, heads, Tq, Tk, D, p)
    H = heads * D
    q, k, _, _, km = AR.make_inputs(family, B, heads, Tq, Tk, D, seed=idx, mask_offset=idx)
    g = torch.Generator().manual_seed(idx)
    bufq = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g))
    bufk = AR.bf16(torch.randn(B, Tk, 3 * H + 8, generator=g))
    bufq[:, :, :H], bufk[:, :, H:2 * H] = q, k
    q_, k_, km_ = bufq.to(DEV)[:, :, :H], bufk.to(DEV)[:, :, H:2 * H], km.to(DEV)
    keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
    ref, budget = PR.reference(q, k, km, heads, D, keep=keep, p=p)
    n = B * heads * Tq * Tk
    worst = 0.0
    for off in ((0, 1) if Tk % 4 == 0 else (0,)):
        raw = torch.full((4 + n + GUARD,), SENTINEL32, dtype=torch.int32, device=DEV)
        lo = 4 + off
        out = raw[lo:lo + n].view(torch.float32).view(B, heads, Tq, Tk)
        assert (out.data_ptr() % 16 == 0) == (off == 0)
        got = ops.attention_probs(q_, k_, km_, heads, D, p_drop=p, site=SITE, seed=SEED, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        host = raw.cpu()
        tag = "%s [output offset %d]" % (what, off)
        assert bool((host[:lo] == SENTINEL32).all()) and bool((host[lo + n:] == SENTINEL32).all()), "%s: elements outside the output overwritten" % tag
        never = host[lo:lo + n] == SENTINEL32
        assert not bool(never.any()), "%s: %d output elements never written" % (tag, int(never.sum()))
        res = host[lo:lo + n].view(torch.float32).view(B, heads, Tq, Tk)
        worst = max(worst, PR.assert_within(res, ref, budget, tag))
        if keep is not None:
            assert bool((res[~torch.as_tensor(keep).reshape(B, heads, Tq, Tk)] == 0.0).all()), "%s: a dropped element is not exactly 0" % tag
    return worst


# 17 x 33: rows that are not 16-byte aligned (dword stores); the others run at an aligned output (float4 stores) and one element further
@pytest.mark.parametrize("Tq,Tk,B", [(17, 36, 5), (17, 33, 5), (124, 44, 5), (512, 300, 2)])
def test_attention_maps_at_head_size_128_against_fp64(Tq, Tk, B):
    worst = 0.0
    for i, (family, p) in enumerate((("masks", 0.0), ("masks", 0.1), ("late_max", 0.0))):
        worst = max(worst, _run_probs(family, B, 2, Tq, Tk, p, 400 + Tq + i))
    print("attention_probs d=128 %dx%d: largest |got - fp64| / budget %.2f" % (Tq, Tk, worst))


def test_attention_maps_still_refuse_head_size_72():
    with pytest.raises(RuntimeError, match="head size 72"):
        ops.attention_probs(torch.zeros(1, 4, 72, device=DEV, dtype=torch.bfloat16), torch.zeros(1, 4, 72, device=DEV, dtype=torch.bfloat16),
                            torch.ones(1, 4, device=DEV, dtype=torch.uint8), 1, 72)


# ------------------------------------------------------------------------------------------- fp8 copies
@pytest.mark.parametrize("Tq,Tk", [(36, 36), (124, 44)])
def test_fp8_copies_of_context_and_gradients_at_head_size_128(Tq, Tk):
    """ops.attention_fwd_q / _bwd_q (tests/test_kernels_gpu.py test_attention_fp8_copies_of_context_and_gradients): the bf16 outputs are
    bit-equal to the plain calls, the e4m3 / e5m2 copies are the host quantisation of those bf16 values with the given scale, the maxima are
    max |bf16 output|; also with the forward's row statistics."""
    B, h, d = 3, 2, D
    g = torch.Generator().manual_seed(Tq * 1000 + Tk + d)
    q, k, v = (torch.randn(B, T, h * d, generator=g).to(DEV).bfloat16() for T in (Tq, Tk, Tk))
    do = (torch.randn(B, Tq, h * d, generator=g) * 1e-3).to(DEV).bfloat16()
    km = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    km[:, Tk - 3:] = 0
    kw = dict(p_drop=0.1, site=3, seed=9)
    assert L.load().crct_attention_quant_ok(Tq, Tk, d) == 1
    ctx = ops.attention_fwd(q, k, v, km, h, d, **kw)
    sc, am = torch.tensor([37.0], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
    ctx2, ctx8 = ops.attention_fwd_q(q, k, v, km, h, d, sc, am, **kw)
    assert torch.equal(ctx, ctx2)
    assert torch.equal(ctx8.view(torch.float8_e4m3fn).float(), (ctx.float() * 37.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float())
    assert float(am.max()) == float(ctx.float().abs().max())
    lse = torch.empty(B, h, Tq, device=DEV)
    assert torch.equal(ops.attention_fwd(q, k, v, km, h, d, row_lse=lse, **kw), ctx)
    for stats in (dict(), dict(row_lse=lse, ctx=ctx)):
        grads = ops.attention_bwd(q, k, v, km, do, h, d, **kw, **stats)
        s1, a1 = torch.tensor([3.0e5], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
        s2, a2 = torch.tensor([1.0e5], device=DEV), torch.zeros(L.FP8_AMAX_LANES, device=DEV)
        grads2, grads8 = ops.attention_bwd_q(q, k, v, km, do, h, d, s1, a1, s2, a2, **kw, **stats)
        for t, t2, t8, s in zip(grads, grads2, grads8, (3.0e5, 1.0e5, 1.0e5)):
            assert torch.equal(t, t2)
            assert float(t.float().abs().max()) > 0
            assert torch.equal(t8.view(torch.float8_e5m2).float(), (t.float() * s).clamp(-57344, 57344).to(torch.float8_e5m2).float())
        assert float(a1.max()) == float(grads[0].float().abs().max())
        assert float(a2.max()) == max(float(grads[1].float().abs().max()), float(grads[2].float().abs().max()))


# ------------------------------------------------------------------------------------------- limits
def test_the_limits_at_head_size_128():
    km = torch.ones(1, 513, dtype=torch.uint8, device=DEV)
    long_q = torch.zeros(1, 513, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="512"):
        ops.attention_fwd(long_q, long_q[:, :20], long_q[:, :20], km[:, :20], 1, 128)
    with pytest.raises(RuntimeError, match="512"):
        ops.attention_probs(long_q, long_q[:, :20], km[:, :20], 1, 128)
    x = torch.zeros(1, 20, 96, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="attention"):
        ops.attention_fwd(x, x, x, km[:, :20], 1, 96)
    with pytest.raises(RuntimeError, match="head size 96"):
        ops.attention_probs(x, x, km[:, :20], 1, 96)
