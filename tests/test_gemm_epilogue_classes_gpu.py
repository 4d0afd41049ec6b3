"""The epilogue classes of the LDS-DMA GEMM kernels (csrc/gemm.hip, epilogue_class / gemm_epilogue_class), -m gpu.

Every configuration that is built with the classes runs every class it is built with, on the smallest shape that reaches every
guard of the batched walk: one full tile plus one partial tile in both directions, an 8-column remainder, two K tiles.  (Configuration
3 is built without them: its cases check that such a configuration runs the generic epilogue whatever the class.)  Each case is one
launch, and
  (a) the output, preact_out and rowsum_out are bitwise what the same launch gives under crct_gemm_force_generic(2), which keeps the
      kernel and runs the generic epilogue;
  (b) they agree per element with the fp64 reference of tests/gemm_ref.py, under the tolerance tests/test_kernels_gpu.py uses for
      the feature: bit for bit where the arithmetic is exact on exact operands (bias, dropout, addends, accumulate, row sums), one
      bf16 step (+ 2^-20 of the terms) behind GELU and GELU';
  (c) every tensor lives in a sentinel canvas with a padded leading dimension of its own (ldc = N + 8, ld_add = N + 16,
      ld_aux = N + 24) and the sentinels are untouched;
  (d) the launch log shows the configuration (and split) that was asked for.
"""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import dropout_ref as DR         # noqa: E402
import gemm_ref as GR            # noqa: E402

DEV = "cuda"
SENT = -1.5 * 2.0 ** 100         # exact in bf16 and fp32; no result comes near it
UNIT = 2.0 ** -12
P_DROP, DROP_SITE, DROP_SEED = 0.1, 29, (1 << 40) + 0x2F1D

# (name, configuration, M, N, K, split_k)
SHAPES = [("cfg15", 15, 200, 72, 128, 0), ("cfg4", 4, 200, 136, 128, 0), ("cfg3", 3, 80, 72, 128, 0), ("cfg50", 50, 264, 136, 128, 0),
          ("cfg15-splitk2", 15, 200, 72, 256, 2)]
# class forms: (name, layout); RESID in its three forms
FORMS = [("plain", "nt"), ("plain-nobias", "nt"), ("gelu-preact", "nt"), ("resid-f32-f32", "nt"), ("resid-bf16-f32", "nt"),
         ("resid-bf16-bf16", "nt"), ("resid-nodrop", "nt"), ("plain", "tb"), ("dgelu", "tb"), ("addend16", "tb")]


def bf(t):
    return t.to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _canvas(M, N, ld, dtype, inner=None, extra_rows=3):
    buf = torch.full((M + extra_rows, ld), SENT, device=DEV, dtype=dtype)
    if inner is not None:
        buf[:M, :N] = inner.to(dtype)
    return buf


def _assert_canary(buf, M, N, what):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:M, :N] = False
    bad = buf[mask].double() != SENT
    assert not bool(bad.any()), "%s: %d elements outside [%d, %d] were written" % (what, int(bad.sum()), M, N)


def _assert_bits(got, ref, what):
    g, r = got.double(), ref.double().to(got.device)
    bad = g != r
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ from the exact result, first at %s (got %r, exact %r)"
                             % (what, int(bad.sum()), bad.numel(), i, float(g[i]), float(r[i])))


def _assert_within_bf16_step(got, ref, scale, what):
    """tests/test_kernels_gpu.py _assert_within_bf16_step: one bf16 step at max(|got|, |ref|) + 2^-20 * scale."""
    got, ref, scale = got.double().cpu(), ref.double().cpu(), scale.double().cpu()
    step = torch.exp2(torch.floor(torch.log2(torch.maximum(got.abs(), ref.abs()).clamp_min(2.0 ** -126))) - 7)
    bad = (got - ref).abs() > step + 2.0 ** -20 * scale
    assert not bool(bad.any()), "%s: %d elements beyond one bf16 step, first at %s (got %r, fp64 %r)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]))


def _logged(fn):
    lib = L.load()
    lib.crct_launch_log_enable(1)
    try:
        fn()
    finally:
        recs = []
        for i in range(lib.crct_launch_log_count()):
            r = L.LaunchRec()
            lib.crct_launch_log_read(i, C.byref(r))
            recs.append((r.cfg, r.split_k, r.n_problems))
        lib.crct_launch_log_enable(0)
    return recs


@functools.lru_cache(maxsize=None)
def _case(layout, M, N, K):
    """Operands (|acc| up to ~12, typically ~0.3: GELU is not trivial), the exact product and the side tensors of one shape; computed
    once and shared by the forms -- nobody writes to them."""
    a, b = GR.operands(M, N, K, 16, 16, seed=M + N + K, ea=-6, eb=-6, extra=1 << 16)
    a, b = a.to(DEV), b.to(DEV)
    acc = GR.ref_nt(a, b)
    if layout == "nt":
        A, B, kw = GR.strided(a, K + 16), GR.strided(b, K + 8), dict(lda=K + 16, ldb=K + 8)
    else:
        A, B, kw = GR.strided(a, K + 16), GR.strided(b.t(), N + 8), dict(tb=True, lda=K + 16, ldb=N + 8)
    g = torch.Generator(device="cpu").manual_seed(13)
    side = dict(bias=GR.unit_ints((N,), 255, 1, UNIT * 4).to(DEV),
                add_b=GR.unit_ints((M, N), 255, 2, UNIT * 8).to(DEV),            # bf16-exact: <= 8 significant bits
                add_f=GR.unit_ints((M, N), 255, 3, UNIT).to(DEV) * 33,           # fp32 only
                src=bf((torch.randn(M, N, generator=g) * 1.5).to(DEV)).double(),
                keep=torch.from_numpy(DR.keep_rowmajor(DROP_SEED, DROP_SITE, M, N, P_DROP)).to(DEV))
    return bf(A), bf(B), kw, acc, side


def _launch(form, A, B, M, N, K, kw, side):
    """One launch of `form` into fresh canvases: ({name: (canvas, is an output)}, launch-log records)."""
    out_f32 = form in ("resid-f32-f32", "resid-bf16-f32")
    t = {"y": (_canvas(M, N, N + 8, torch.float32 if out_f32 else torch.bfloat16), True)}
    args = dict(out=t["y"][0], ldc=N + 8)
    drop = dict(p_drop=P_DROP, site=DROP_SITE, seed=DROP_SEED)
    if form in ("plain", "gelu-preact") or form.startswith("resid"):
        if kw.get("tb") is None:
            args["bias"] = side["bias"].float()
    if form == "gelu-preact":
        t["pre"] = (_canvas(M, N, N + 24, torch.bfloat16), True)
        args.update(act="gelu", preact_out=t["pre"][0], ld_aux=N + 24)
    elif form.startswith("resid"):
        f32_add = form == "resid-f32-f32"
        t["add"] = (_canvas(M, N, N + 16, torch.float32 if f32_add else torch.bfloat16, inner=side["add_f" if f32_add else "add_b"]), False)
        args.update(addend=t["add"][0], ld_add=N + 16, c_cached=out_f32)
        if form != "resid-nodrop":
            args.update(drop)
    elif form == "dgelu":
        t["src"] = (_canvas(M, N, N + 24, torch.bfloat16, inner=side["src"]), False)
        args.update(dact_src=t["src"][0], dact="gelu", ld_aux=N + 24)
    elif form == "addend16":
        t["add"] = (_canvas(M, N, N + 16, torch.bfloat16, inner=side["add_b"]), False)
        args.update(addend=t["add"][0], ld_add=N + 16)
    recs = _logged(lambda: ops.gemm(A, B, M, N, K, **args, **kw))
    torch.cuda.synchronize()
    return t, recs


def _reference(form, acc, side, tb):
    bias = None if (tb or form == "plain-nobias") else side["bias"]
    if form in ("plain", "plain-nobias"):
        return GR.epilogue(acc, bias=bias)
    if form == "gelu-preact":
        return GR.epilogue(acc, bias=bias, act="gelu")
    if form == "dgelu":
        return GR.epilogue(acc, dact="gelu", dact_src=side["src"])
    if form == "addend16":
        return GR.epilogue(acc, addend=side["add_b"])
    drop = {} if form == "resid-nodrop" else dict(keep=side["keep"], drop_scale=1.0 / (1.0 - P_DROP))
    return GR.epilogue(acc, bias=bias, addend=side["add_f" if form == "resid-f32-f32" else "add_b"],
                       out="f32" if form in ("resid-f32-f32", "resid-bf16-f32") else "bf16", **drop)


@pytest.mark.parametrize("form,layout", FORMS, ids=["%s-%s" % f for f in FORMS])
@pytest.mark.parametrize("name,cfg,M,N,K,split", SHAPES, ids=[s[0] for s in SHAPES])
def test_epilogue_class_equals_the_generic_epilogue_and_fp64(name, cfg, M, N, K, split, form, layout):
    lib = L.load()
    A, B, kw, acc, side = _case(layout, M, N, K)
    kw = dict(kw, tile=cfg, split_k=split)
    what = "%s %s %s" % (name, layout, form)
    try:
        lib.crct_gemm_force_generic(0)
        got, recs = _launch(form, A, B, M, N, K, kw, side)
        lib.crct_gemm_force_generic(2)
        gen, recs_gen = _launch(form, A, B, M, N, K, kw, side)
    finally:
        lib.crct_gemm_force_generic(0)
    # (d) the configuration that was asked for, in both runs
    expect = [(cfg, split if split else 1, 1)]
    assert recs == expect and recs_gen == expect, (what, recs, recs_gen, expect)
    # (a) bitwise the generic epilogue's result, sentinels included
    for k, (buf, _) in got.items():
        assert torch.equal(_bits(buf), _bits(gen[k][0])), "%s: %s differs from the generic epilogue's" % (what, k)
    # (c) sentinels
    for k, (buf, _) in got.items():
        _assert_canary(buf, M, N, what + ": " + k)
    # (b) fp64
    r = _reference(form, acc, side, layout == "tb")
    y = got["y"][0][:M, :N]
    if form == "gelu-preact":
        _assert_bits(got["pre"][0][:M, :N], r["pre"], what + ": preact_out")
        _assert_within_bf16_step(y, r["v"], r["v"].abs(), what)
    elif form == "dgelu":
        s = side["src"]
        terms = 0.5 * (1 + torch.erf(s / math.sqrt(2)).abs()) + (s * torch.exp(-0.5 * s * s)).abs() / math.sqrt(2 * math.pi)
        _assert_within_bf16_step(y, r["v"], acc.abs() * terms, what)
    else:
        _assert_bits(y, r["y"], what)
    # the inputs inside their canvases are what they were
    for k, key in (("add", "add_f" if form == "resid-f32-f32" else "add_b"), ("src", "src")):
        if k in got:
            _assert_bits(got[k][0][:M, :N], side[key], what + ": input " + k)


@functools.lru_cache(maxsize=None)
def _wgrad_case(M, N, R, seed):
    a, b = GR.operands(M, N, R, 32, 32, seed, ea=-3, eb=-5, extra=1 << 14)
    a, b = a.to(DEV), b.to(DEV)
    A, B = bf(GR.strided(a.t(), M + 8)), bf(GR.strided(b.t(), N + 8))
    pre = GR.unit_ints((M, N), 64, seed + 1, 2.0 ** -8).to(DEV)
    rs_pre = GR.unit_ints((M,), 64, seed + 2, 2.0 ** -3).to(DEV)
    return A, B, dict(ta=True, tb=True, lda=M + 8, ldb=N + 8), GR.ref_nt(a, b), pre, rs_pre, rs_pre + A[:R, :M].double().sum(0)


# crct_gemm_bf16_grouped groups problems of more than 96 rows only: the pair 136 x 72 / 72 x 136 is launched one by one (weight gradients
# of that size on configuration 3, which is built without the classes), the pair 136 x 72 / 200 x 136 as ONE grid of configuration 4
# with the WGRAD class
WGRAD_PAIRS = [("72-row-second", ((136, 72), (72, 136)), [(3, 1, 1), (3, 1, 1)]), ("grouped", ((136, 72), (200, 136)), [(4, 1, 2)])]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("pair,shapes,expect", WGRAD_PAIRS, ids=[p[0] for p in WGRAD_PAIRS])
def test_weight_gradient_class_grouped(pair, shapes, expect, accumulate):
    """WGRAD: two problems over 192 tokens handed to one grouped call, fp32 outputs written or accumulated, with the bias gradient
    (rowsum_out) from the same kernel."""
    lib = L.load()
    R = 192
    cases = [_wgrad_case(M, N, R, 5 + 4 * i) for i, (M, N) in enumerate(shapes)]

    def launch():
        probs, bufs = [], []
        for (A, B, kw, ref, pre, rs_pre, rs_ref) in cases:
            M, N = ref.shape
            out = _canvas(M, N, N + 8, torch.float32, inner=pre)
            rs = torch.full((M + 8,), SENT, device=DEV)
            rs[:M] = rs_pre.float()
            probs.append(dict(A=A, B=B, M=M, N=N, K=R, out=out, ldc=N + 8, accumulate=accumulate, rowsum_out=rs, **kw))
            bufs.append((out, rs))
        recs = _logged(lambda: ops.gemm_grouped(probs))
        torch.cuda.synchronize()
        return bufs, recs

    try:
        lib.crct_gemm_force_generic(0)
        got, recs = launch()
        lib.crct_gemm_force_generic(2)
        gen, recs_gen = launch()
    finally:
        lib.crct_gemm_force_generic(0)
    assert recs == expect and recs_gen == expect, (recs, recs_gen, expect)
    for i, ((out, rs), (out_g, rs_g), (A, B, kw, ref, pre, rs_pre, rs_ref)) in enumerate(zip(got, gen, cases)):
        M, N = ref.shape
        what = "%s problem %d %s" % (pair, i, "accumulate" if accumulate else "overwrite")
        assert torch.equal(_bits(out), _bits(out_g)) and torch.equal(_bits(rs), _bits(rs_g)), what + ": differs from the generic epilogue's"
        _assert_bits(out[:M, :N], GR.f32(ref + pre) if accumulate else GR.f32(ref), what)
        _assert_bits(rs[:M], rs_ref, what + ": rowsum_out")
        assert bool((rs[M:] == SENT).all()), what + ": rowsum_out written past M"
        _assert_canary(out, M, N, what)
