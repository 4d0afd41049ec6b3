"""Every attention kernel per element against fp64 (-m gpu): csrc/attention_mfma.hip (all 75 (query tiles, key tiles, head size) triples,
one wave and cooperating waves per pair), csrc/attention.hip (fp32 VALU, all nine tile classes) and csrc/attention_long.hip (4 / 8 waves,
resident / shared images, kept / recomputed statistics, the dropout-bit cache on and off, odd key-tile counts).

Every case runs the way the step engine calls the kernels: q, k, v are column slices of fused [*, 3 H + 8] buffers, dq goes into slice 0
of a [B, Tq, 3 H] buffer, dk / dv into slices 1 / 2 of a [B, Tk, 3 H] buffer, ctx into a buffer of leading dimension H + 8.  The
output buffers are filled with a sentinel and followed by guard rows: after the call every element outside the output slices must
still hold it.  The outputs are compared per element with the fp64 reference of tests/attention_ref.py under its derived budget (the
yardstick tests/test_attention_ref_cpu.py proves); the dropout mask is the host Philox copy's (tests/dropout_ref.py).

Largest |got - fp64| / (bf16 step + budget) measured on the MI355X (each test prints its own; run with -s): MFMA sweep 0.87 (dv, d = 32),
VALU sweep 0.38 (dk, d = 64), long kernels 0.70 (dv, 1 x 113 x 32), the hard families 0.70 (ctx, late_max) -- the emulator's figures
(tests/test_attention_ref_cpu.py) to two digits: the kernels round where their headers say and nowhere else.
"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import attention_ref as AR        # noqa: E402
import dropout_ref as DR          # noqa: E402

DEV = "cuda"
SEED, SITE = 20240917, 11
SENTINEL = 0x7B7B                 # bf16 bit pattern (1.3e36) no attention output takes
GUARD_ROWS = 3


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
        assert not bool(touched.any()), "%s: %d elements outside the output slices overwritten, first at flat index %d (row %d, column %d of ld %d)" % (
            what, int(touched.sum()), int(touched.nonzero()[0]), int(touched.nonzero()[0]) // self.ld, int(touched.nonzero()[0]) % self.ld, self.ld)
        assert not bool((raw[self.written] == SENTINEL).any()), "%s: output elements never written" % what


class _Case:
    """Operands of one case on the device (as slices of fused buffers) with the keep mask; the fp64 reference is made once (`ref`)."""

    def __init__(self, family, B, heads, Tq, Tk, d, p, idx):
        self.B, self.heads, self.Tq, self.Tk, self.d, self.p = B, heads, Tq, Tk, d, p
        self.what = "%s B=%d heads=%d %dx%dx%d p=%g" % (family, B, heads, Tq, Tk, d, p)
        H = self.H = heads * d
        self.q, self.k, self.v, self.dctx, self.km = AR.make_inputs(family, B, heads, Tq, Tk, d, seed=idx, mask_offset=idx)
        g = torch.Generator().manual_seed(idx)
        bufq = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g))        # the neighbours hold data, not zeros: a kernel that strays reads them
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

    def run(self, tag, kept=False, worst=None):
        """Forward and backward into fresh sentinel canvases; per-element budget, intact sentinels, and (kept) row_lse.  Returns the
        largest budget ratio per output (also folded into `worst`)."""
        B, heads, Tq, Tk, d, H, p = self.B, self.heads, self.Tq, self.Tk, self.d, self.H, self.p
        what = "%s [%s%s]" % (self.what, tag, ", kept statistics" if kept else "")
        c_ctx, c_dq, c_dkv = _Canvas(B, Tq, H + 8), _Canvas(B, Tq, 3 * H), _Canvas(B, Tk, 3 * H)
        ctx, dq, dk, dv = c_ctx.view(0, H), c_dq.view(0, H), c_dkv.view(H, H), c_dkv.view(2 * H, H)
        lse = torch.full((B, heads, Tq), float("nan"), device=DEV) if kept else None
        out = ops.attention_fwd(self.q_, self.k_, self.v_, self.km_, heads, d, p_drop=p, site=SITE, seed=SEED, row_lse=lse, out=ctx)
        assert out.data_ptr() == ctx.data_ptr()
        ops.attention_bwd(self.q_, self.k_, self.v_, self.km_, self.do_, heads, d, p_drop=p, site=SITE, seed=SEED, row_lse=lse,
                          ctx=ctx if kept else None, outs=(dq, dk, dv))
        torch.cuda.synchronize()
        ref = self.ref(ctx.cpu() if kept else None)
        got = dict(ctx=ctx.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
        res = {}
        for n in AR.OUTPUTS:
            res[n] = AR.assert_within(got[n], ref[n], AR.budget_of(ref, n, kept), "%s: %s" % (what, n))
        for c, n in ((c_ctx, "ctx"), (c_dq, "dq"), (c_dkv, "dk / dv")):
            c.assert_intact("%s: %s canvas" % (what, n))
        if kept:
            # log2 sum_j exp2(x_ij) against fp64, within fp32 slack at that magnitude
            err = (lse.double().cpu() - ref["lse"]).abs()
            tol = 2.0 ** -16 * (1.0 + ref["lse"].abs())
            bad = err > tol
            assert not bool(bad.any()), "%s: row_lse: %d rows off, first at %s (got %r, fp64 %r)" % (
                what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(lse.cpu()[bad][0]), float(ref["lse"][bad][0]))
        if worst is not None:
            for n, x in res.items():
                worst[n] = max(worst.get(n, 0.0), x)
        return res


def _show(title, worst, n_cases):
    print("%s: %d cases, largest |got - fp64| / budget: " % (title, n_cases) + ", ".join("%s %.2f" % (n, worst.get(n, 0.0)) for n in AR.OUTPUTS))


# ------------------------------------------------------------------------------------------- MFMA and VALU sweep (lengths up to 112)
# one ragged length per tile count 1 - 4; the 7-tile class (65 .. 112 keys: 5, 6 or 7 tiles of data padded to 7) takes 65, 81 and 112 in turn
SHORT = (5, 17, 36, 49)
SEVEN = (65, 81, 112)


def _sweep_lengths():
    """The 25 (Tq, Tk) of {1, 2, 3, 4, 7}^2 tile counts with their case index."""
    out = []
    for iq in range(5):
        for ik in range(5):
            Tq = SHORT[iq] if iq < 4 else SEVEN[(iq + 2 * ik) % 3]
            Tk = SHORT[ik] if ik < 4 else SEVEN[(2 * iq + ik + 1) % 3]
            out.append((5 * iq + ik, Tq, Tk))
    return out


def _tiles(T):
    n = (T + 15) // 16
    return 7 if n > 4 else n


def test_the_sweep_lengths_cover_every_tile_pair_and_all_three_seven_tile_lengths():
    lens = _sweep_lengths()
    assert len({(_tiles(Tq), _tiles(Tk)) for _, Tq, Tk in lens}) == 25
    assert {T for _, Tq, Tk in lens for T in (Tq, Tk)} == set(SHORT + SEVEN)
    valu_class = lambda T: 2 if T <= 32 else (3 if T <= 48 else 7)      # noqa: E731  (attention.hip tile_class)
    assert len({(valu_class(Tq), valu_class(Tk)) for _, Tq, Tk in lens}) == 9


@pytest.mark.parametrize("d", [32, 48, 64])
def test_mfma_every_tile_pair_against_fp64_with_strided_outputs(d):
    """attention_mfma.hip at all 25 tile pairs of this head size (with the other two head sizes: the 75 instantiated triples), each
    with one wave per pair (force_split 1) and with the default cooperating waves (0: 4 waves from 4 x 4 tiles, 2 from 2 x 2).  B = 2,
    heads = 3: six pairs do not fill the workgroups of 4 (or 8) pairs, so the surplus-group path runs.  p alternates 0 / 0.1, the
    input families rotate with the case index."""
    worst, seen = {}, set()
    for idx, Tq, Tk in _sweep_lengths():
        case = _Case(AR.FAMILIES[(idx + d // 16) % 5], 2, 3, Tq, Tk, d, 0.1 * ((idx + d // 16) % 2), idx)
        for split in (1, 0):
            with _hooks(split=split):
                case.run("mfma, force_split %d" % split, worst=worst)
            seen.add((_tiles(Tq), _tiles(Tk), d, split))
    assert len(seen) == 50
    _show("mfma d=%d" % d, worst, len(seen))


@pytest.mark.parametrize("d", [8, 24, 40, 64])
def test_valu_every_tile_class_against_fp64_with_strided_outputs(d):
    """attention.hip (force_valu) at the same 25 length pairs -- all nine CASE(cq, ck) launches -- at head sizes only it takes (8, 24,
    40) and at 64."""
    worst, seen = {}, set()
    for idx, Tq, Tk in _sweep_lengths():
        case = _Case(AR.FAMILIES[(idx + d // 8) % 5], 2, 3, Tq, Tk, d, 0.1 * ((idx + d // 8) % 2), idx)
        with _hooks(valu=1):
            case.run("valu", worst=worst)
        seen.add((Tq, Tk, d))
    assert len(seen) == 25
    _show("valu d=%d" % d, worst, len(seen))


# ------------------------------------------------------------------------------------------- long kernels
LDS_CAP = 160 * 1024


def _long_plan(Tq, Tk, d, p):
    """What attention_long.hip launch_d decides for a shape (waves_for, bwd_lds, bwd_share, keep_cache restated):
    dict(nw_fwd, nw_bwd, share, keep_cache, odd_nk)."""
    NQ, NK, ND = (Tq + 15) // 16, (Tk + 15) // 16, d // 16
    nw_fwd, nw_bwd = (8 if NQ >= 8 else 4), (8 if min(NQ, NK) >= 8 else 4)
    stb = 32 * ND + 16

    def bwd_lds(share):
        rows = 2 * max(NQ, NK) if share else 2 * (NQ + NK)
        return 16 * rows * stb + 256 * NQ + 64 * NK + nw_bwd * 16 * 48

    share = bwd_lds(False) > LDS_CAP
    lds = bwd_lds(share)
    cache = 64 * NQ * NK
    keep_cache = bool(p > 0 and lds + cache <= LDS_CAP and LDS_CAP // (lds + cache) == LDS_CAP // lds)
    return dict(nw_fwd=nw_fwd, nw_bwd=nw_bwd, share=share, keep_cache=keep_cache, odd_nk=bool(NK & 1))


# (Tq, Tk, d, force_long) -- the smallest shapes that reach each branch.  With p = 0.1 the dropout-bit cache (keep_cache) is ON for
# 113 x 113 x 32, 129 x 17, 17 x 129, the three shared-image threshold shapes (the shared images leave room) and the three forced short
# shapes; OFF for 1 x 113, 145 x 129 and the three resident threshold shapes (the cache would cost a workgroup per CU) and for
# 512 x 512 x 64 (its LDS is full).  test_the_long_cases_reach_every_branch pins this against a restatement of the launcher's rules.
LONG_CASES = [
    (113, 113, 32, 0),        # 8 x 8 tiles: 8 waves in both directions
    (129, 17, 48, 0),         # 8 waves forward, 4 backward
    (17, 129, 64, 0),         # 4 waves forward (2 query tiles), 4 backward; odd key-tile count
    (1, 113, 32, 0),
    (145, 129, 48, 0),        # 9 key tiles: the last tile pair of the forward is half absent
    (512, 512, 64, 0),        # the limit: shared images, LDS full
    (445, 443, 32, 0), (461, 449, 32, 0),      # d = 32: 28 x 28 tiles resident (158464 B), 29 x 29 shared (163904 B > 160 KiB)
    (333, 330, 48, 0), (349, 340, 48, 0),      # d = 48: 21 x 21 resident, 22 x 22 shared
    (253, 250, 64, 0), (269, 260, 64, 0),      # d = 64: 16 x 16 resident, 17 x 17 shared
    (5, 5, 48, 1), (20, 36, 32, 1), (112, 112, 64, 1),      # the short shapes through the long kernels (force_long)
]


def test_the_long_cases_reach_every_branch():
    plans = [_long_plan(Tq, Tk, d, 0.1) for Tq, Tk, d, _ in LONG_CASES]
    for key in ("share", "keep_cache", "odd_nk"):
        assert {pl[key] for pl in plans} == {False, True}, key
    assert {(pl["nw_fwd"], pl["nw_bwd"]) for pl in plans} == {(8, 8), (8, 4), (4, 4)}
    by = {(Tq, Tk, d): _long_plan(Tq, Tk, d, 0.1) for Tq, Tk, d, _ in LONG_CASES}
    for res, sh in (((445, 443, 32), (461, 449, 32)), ((333, 330, 48), (349, 340, 48)), ((253, 250, 64), (269, 260, 64))):
        assert not by[res]["share"] and by[sh]["share"]       # one shape on each side of the bwd_share threshold per head size
        assert (sh[0] + 15) // 16 == (res[0] + 15) // 16 + 1 and (sh[1] + 15) // 16 == (res[1] + 15) // 16 + 1
    on = {(113, 113, 32), (129, 17, 48), (17, 129, 64), (461, 449, 32), (349, 340, 48), (269, 260, 64), (5, 5, 48), (20, 36, 32), (112, 112, 64)}
    assert {key for key, pl in by.items() if pl["keep_cache"]} == on
    assert by[(512, 512, 64)]["share"] and {(pl["share"], pl["keep_cache"]) for pl in plans} == {(False, False), (False, True), (True, False), (True, True)}
    assert all(not _long_plan(Tq, Tk, d, 0.0)["keep_cache"] for Tq, Tk, d, _ in LONG_CASES)


@pytest.mark.parametrize("idx", range(len(LONG_CASES)), ids=["%dx%dx%d%s" % (a, b, c, "-forced" if f else "") for a, b, c, f in LONG_CASES])
def test_long_kernels_against_fp64_with_strided_outputs(idx):
    """attention_long.hip at LONG_CASES[idx]: p in {0, 0.1} x {recomputed, kept} statistics, B = 1, heads = 2; with kept statistics also
    row_lse per element against fp64 logsumexp * log2e within 2^-16 (1 + |lse|)."""
    Tq, Tk, d, force = LONG_CASES[idx]
    worst, n = {}, 0
    for ip, p in enumerate((0.0, 0.1)):
        case = _Case(AR.FAMILIES[(idx + ip) % 5], 1, 2, Tq, Tk, d, p, 100 + 2 * idx + ip)
        for kept in (False, True):
            with _hooks(long=force):
                case.run("long", kept=kept, worst=worst)
            n += 1
    _show("long %dx%dx%d%s" % (Tq, Tk, d, " (forced)" if force else ""), worst, n)


# ------------------------------------------------------------------------------------------- the hard families on every path
@pytest.mark.parametrize("family", ["late_max", "early_max", "masks"])
def test_hard_families_on_every_path(family):
    """late_max (the row maximum arrives with the last attended key), early_max and masks (a random 70 %, every key masked, one key
    attended in the last tile, an aligned tile pair masked in the middle: B = 4 gives every kind) at one short, one 7-tile and one long
    shape, forward and backward, p = 0.1: MFMA with one wave and cooperating waves, VALU, the long kernels forced onto the short
    shapes and by themselves on the long one, recomputed and kept statistics."""
    worst, n = {}, 0
    for i, (Tq, Tk, d) in enumerate(((20, 36, 32), (100, 81, 48), (145, 200, 64))):
        case = _Case(family, 4, 2, Tq, Tk, d, 0.1, 200 + i)
        runs = [("long", dict(long=1), False), ("long", dict(long=1), True)]
        if Tq <= 112 and Tk <= 112:
            runs += [("mfma, force_split 1", dict(split=1), False), ("mfma", dict(), False), ("valu", dict(valu=1), False)]
        for tag, hooks, kept in runs:
            with _hooks(**hooks):
                case.run(tag, kept=kept, worst=worst)
            n += 1
    _show("family %s" % family, worst, n)


def test_caller_supplied_outputs_are_checked_and_the_defaults_unchanged():
    """out= / outs= of the wrappers: a strided view gives the same bits as the default contiguous output; a view the kernels cannot
    address (wrong shape, batches that do not follow one another) is refused."""
    case = _Case("flat", 2, 3, 20, 36, 32, 0.1, 7)
    H = case.H
    args = (case.q_, case.k_, case.v_, case.km_, 3, 32)
    kw = dict(p_drop=0.1, site=SITE, seed=SEED)
    ctx0 = ops.attention_fwd(*args, **kw)
    g0 = ops.attention_bwd(*args[:4], case.do_, 3, 32, **kw)
    assert ctx0.is_contiguous() and all(t.is_contiguous() for t in g0)
    c = _Canvas(2, 20, H + 8)
    assert torch.equal(ops.attention_fwd(*args, out=c.view(0, H), **kw), ctx0)
    cq, ck = _Canvas(2, 20, 3 * H), _Canvas(2, 36, 3 * H)
    g1 = ops.attention_bwd(*args[:4], case.do_, 3, 32, outs=(cq.view(0, H), ck.view(H, H), ck.view(2 * H, H)), **kw)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="attention_fwd: out"):
        ops.attention_fwd(*args, out=torch.empty(2, 21, H, device=DEV, dtype=torch.bfloat16), **kw)
    with pytest.raises(RuntimeError, match="attention_fwd: out"):
        ops.attention_fwd(*args, out=torch.empty(2, 24, H + 8, device=DEV, dtype=torch.bfloat16)[:, :20, :H], **kw)

