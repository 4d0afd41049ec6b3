"""The LayerNorm addend of the GEMM epilogues (CrctGemmLnAddend; csrc/gemm.hip, common.hip.h ln_value) and the step engine's use of it
(crct_engine_set_ln_addend), -m gpu.

The block-closing GEMMs of the fp32 residual stream add the fp32 output of the LayerNorm that produced their block's input.  That value
is either read from a copy the LayerNorm wrote (CrctLnFwdArgs.y_f32, CrctGemmArgs.addend_f32) or rebuilt in the epilogue from the
LayerNorm's own inputs: y32[m][n] = gamma[n] * ((s[m][n] - mean[m]) * rstd[m]) + beta[n].  Both spell the value through one device
function, so
  * kernel, bit for bit: the same GEMM with the fp32 addend `layernorm_fwd(..., y_f32=True)` wrote and with the new addend built from
    that call's inputs and returned statistics gives torch.equal outputs, fp32 and bf16 -- configurations 15 and 12 (RESID class), 4
    and 3 (generic epilogue), split-K, the grouped launcher and the register-staged kernel, rows and columns that end inside a tile,
    ld_add > N, dropout on and off, with bias; the output canvases' sentinels are untouched;
  * kernel against fp64, per element: with operands, side tensors and LayerNorm inputs on power-of-two grids every fp32 operation of
    the epilogue is either exact or ONE rounding of an exactly known value, which fp64 reproduces -- bit for bit, the tolerance of the
    RESID checks of tests/test_gemm_epilogue_classes_gpu.py;
  * engine: every step output, tap and gradient of a step with crct_engine_set_ln_addend 1 equals the step with 0 bit for bit.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as CFG, ops, lib as L, synthetic as S   # noqa: E402
from crct.model import VisualDialogEncoder                      # noqa: E402
from crct.step_adapter import forward as step_forward           # noqa: E402
import dropout_ref as DR         # noqa: E402
import gemm_ref as GR            # noqa: E402

DEV = "cuda"
SENT = -1.5 * 2.0 ** 100         # exact in bf16 and fp32; no result comes near it
P_DROP, DROP_SITE, DROP_SEED = 0.1, 31, (1 << 40) + 0x51A7
MS, NS, KS = (1, 127, 129, 257), (72, 200, 768), (64, 192)
CONFIGS = (15, 12, 4, 3)         # 15 / 12: built with the epilogue classes (RESID); 4 in a single launch too; 3: the generic epilogue


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
    assert bool((buf[mask].double() == SENT).all()), "%s: elements outside [%d, %d] were written" % (what, M, N)


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
def _ln_case(M, N):
    """The LayerNorm of M fp32 rows of width N through the library's kernel: its inputs, the statistics it returned and the fp32 output
    it wrote, the two addends inside canvases of leading dimension N + 16.  Shared by the cases; nobody writes to them."""
    g = torch.Generator(device="cpu").manual_seed(1000 * M + N)
    s = (torch.randn(M, N, generator=g) * 1.7 + 0.3).to(DEV)
    gamma = (1.0 + 0.25 * torch.randn(N, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(N, generator=g)).to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    _, mean, rstd, y32 = ops.layernorm_fwd(s, gamma, beta, y_f32=True)
    torch.cuda.synchronize()
    return dict(s=_canvas(M, N, N + 16, torch.float32, inner=s), y32=_canvas(M, N, N + 16, torch.float32, inner=y32),
                ln=(mean, rstd, gamma, beta), bias=bias)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(7 * M + 3 * N + K)
    A = torch.randn(M, K + 16, generator=g).to(torch.bfloat16).to(DEV)
    B = (torch.randn(N, K + 8, generator=g) * 0.2).to(torch.bfloat16).to(DEV)
    return A, B


def _both_addends(M, N, K, out_f32, drop, **kw):
    """One GEMM y = dropout(A B^T + bias) + addend twice, into fresh canvases: (with the LayerNorm's fp32 copy, with the LayerNorm
    addend, launch-log records of the second)."""
    A, B = _operands(M, N, K)
    c = _ln_case(M, N)
    dt = torch.float32 if out_f32 else torch.bfloat16
    common = dict(lda=K + 16, ldb=K + 8, ldc=N + 8, bias=c["bias"], ld_add=N + 16, c_cached=out_f32, **kw)
    if drop:
        common.update(p_drop=P_DROP, site=DROP_SITE, seed=DROP_SEED)
    ref, got = _canvas(M, N, N + 8, dt), _canvas(M, N, N + 8, dt)
    ops.gemm(A, B, M, N, K, out=ref, addend=c["y32"], **common)
    recs = _logged(lambda: ops.gemm(A, B, M, N, K, out=got, addend=c["s"], ln_addend=c["ln"], **common))
    torch.cuda.synchronize()
    return ref, got, recs


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_ln_addend_equals_the_fp32_copy_bit_for_bit(cfg, M):
    for N in NS:
        for K in KS:
            for out_f32 in (True, False):
                for drop in (True, False):
                    what = "cfg %d  %d x %d x %d  out %s  dropout %s" % (cfg, M, N, K, "fp32" if out_f32 else "bf16", drop)
                    ref, got, recs = _both_addends(M, N, K, out_f32, drop, tile=cfg)
                    assert recs == [(cfg, 1, 1)], (what, recs)
                    assert torch.equal(_bits(got), _bits(ref)), what
                    assert bool((got[:M, :N].double() != SENT).all()), what
                    _assert_canary(got, M, N, what)


@pytest.mark.parametrize("cfg", (15, 12, 4))
def test_ln_addend_split_k_last_arriver(cfg):
    """S = 2: the workgroup that arrives last reduces the slabs and runs the epilogue with the LayerNorm addend."""
    M, N, K = 129, 200, 256
    for out_f32 in (True, False):
        ref, got, recs = _both_addends(M, N, K, out_f32, True, tile=cfg, split_k=2)
        assert recs == [(cfg, 2, 1)], recs
        assert torch.equal(_bits(got), _bits(ref)), (cfg, out_f32)
        _assert_canary(got, M, N, "split-K cfg %d" % cfg)


def test_ln_addend_register_staged_kernel():
    """K = 72 is no multiple of 64: the register-staged kernel and its per-lane epilogue."""
    M, N, K = 129, 72, 72
    for out_f32 in (True, False):
        ref, got, recs = _both_addends(M, N, K, out_f32, True)
        assert recs and recs[0][0] >= 16, recs       # launch-log ids 16 .. 19: the register-staged kernel's tiles
        assert torch.equal(_bits(got), _bits(ref)), out_f32
        _assert_canary(got, M, N, "register-staged")


def test_ln_addend_grouped_launch():
    """Two forward problems in ONE grid (configuration 9, generic epilogue), the second without a LayerNorm addend of its own."""
    shapes = [(129, 200, 192), (257, 72, 192)]

    def launch(use_ln):
        probs, outs = [], []
        for i, (M, N, K) in enumerate(shapes):
            A, B = _operands(M, N, K)
            c = _ln_case(M, N)
            out = _canvas(M, N, N + 8, torch.float32)
            p = dict(A=A, B=B, M=M, N=N, K=K, out=out, lda=K + 16, ldb=K + 8, ldc=N + 8, bias=c["bias"], ld_add=N + 16, c_cached=True,
                     p_drop=P_DROP, site=DROP_SITE + i, seed=DROP_SEED, addend=c["y32"])
            if use_ln and i == 0:
                p.update(addend=c["s"], ln_addend=c["ln"])
            probs.append(p)
            outs.append(out)
        recs = _logged(lambda: ops.gemm_grouped(probs))
        torch.cuda.synchronize()
        return outs, recs

    ref, _ = launch(False)
    got, recs = launch(True)
    assert recs == [(9, 1, 2)], recs
    for (M, N, K), r, g in zip(shapes, ref, got):
        assert torch.equal(_bits(g), _bits(r)), (M, N, K)
        _assert_canary(g, M, N, "grouped %d x %d" % (M, N))


def test_ln_addend_grouped_call_launched_one_by_one():
    """A grouped call that does not qualify for one grid (a problem of 96 rows) runs as single launches, and each problem takes its
    own LayerNorm addend along: the launches and the bits of the two single ``ops.gemm`` calls."""
    shapes = [(96, 72, 64), (129, 200, 64)]

    def problems():
        probs, outs = [], []
        for i, (M, N, K) in enumerate(shapes):
            A, B = _operands(M, N, K)
            c = _ln_case(M, N)
            out = _canvas(M, N, N + 8, torch.float32)
            p = dict(A=A, B=B, M=M, N=N, K=K, out=out, lda=K + 16, ldb=K + 8, ldc=N + 8, bias=c["bias"], ld_add=N + 16, c_cached=True,
                     p_drop=P_DROP, site=DROP_SITE + i, seed=DROP_SEED, addend=c["y32"])
            if i == 0:
                p.update(addend=c["s"], ln_addend=c["ln"])
            probs.append(p)
            outs.append(out)
        return probs, outs

    probs, ref = problems()
    single = _logged(lambda: [ops.gemm(**p) for p in probs])
    probs, got = problems()
    recs = _logged(lambda: ops.gemm_grouped(probs))
    torch.cuda.synchronize()
    assert len(recs) == 2 and all(r[2] == 1 for r in recs) and recs == single, (recs, single)
    for (M, N, K), r, g in zip(shapes, ref, got):
        assert torch.equal(_bits(g), _bits(r)), (M, N, K)
        assert bool((g[:M, :N].double() != SENT).all()), (M, N, K)
        _assert_canary(g, M, N, "one by one %d x %d" % (M, N))


def test_ln_addend_is_refused_without_its_fp32_rows():
    M, N, K = 129, 72, 64
    A, B = _operands(M, N, K)
    c = _ln_case(M, N)
    with pytest.raises(RuntimeError):            # a bf16 addend cannot be the rows of a LayerNorm addend
        ops.gemm(A, B, M, N, K, lda=K + 16, ldb=K + 8, addend=c["s"].to(torch.bfloat16), ld_add=N + 16, ln_addend=c["ln"])
    with pytest.raises(RuntimeError):            # ... nor can no addend at all
        ops.gemm(A, B, M, N, K, lda=K + 16, ldb=K + 8, ln_addend=c["ln"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ fp64, per element
UNIT = 2.0 ** -12


@functools.lru_cache(maxsize=None)
def _exact_case(M, N, K):
    """Everything on grids: the product is exact (tests/gemm_ref.py); s - mean is exact, (s - mean) * rstd is exact (rstd a power of
    two), gamma * t and gamma * t + beta are exact in fp64, so the kernel's single fused multiply-add rounds the value fp64 holds; the
    sum with the (rounded) dropout result is one more fp32 rounding of an fp64-exact sum."""
    a, b = GR.operands(M, N, K, 16, 16, seed=M + N + K, ea=-6, eb=-6, extra=1 << 16)
    a, b = a.to(DEV), b.to(DEV)
    s = GR.unit_ints((M, N), 255, 3, UNIT).to(DEV) * 33
    mean = GR.unit_ints((M,), 255, 4, UNIT * 8).to(DEV)
    rstd = torch.exp2(GR.ints((M,), 3, 5)).to(DEV)                     # 1/8 .. 8
    gamma = GR.unit_ints((N,), 255, 6, 2.0 ** -7).to(DEV)
    beta = GR.unit_ints((N,), 255, 7, UNIT * 4).to(DEV)
    bias = GR.unit_ints((N,), 255, 1, UNIT * 4).to(DEV)
    keep = torch.from_numpy(DR.keep_rowmajor(DROP_SEED, DROP_SITE, M, N, P_DROP)).to(DEV)
    t = GR.f32(GR.f32(s - mean[:, None]) * rstd[:, None])
    ln = GR.f32(gamma[None, :] * t + beta[None, :])
    return a, b, GR.ref_nt(a, b), dict(s=s, mean=mean, rstd=rstd, gamma=gamma, beta=beta, bias=bias, keep=keep, ln=ln)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_ln_addend_against_fp64_per_element(cfg):
    M, N, K = 129, 200, 192
    a, b, acc, side = _exact_case(M, N, K)
    A = GR.strided(a, K + 16).to(torch.bfloat16)
    B = GR.strided(b, K + 8).to(torch.bfloat16)
    ln = tuple(side[k].float().contiguous() for k in ("mean", "rstd", "gamma", "beta"))
    s = _canvas(M, N, N + 16, torch.float32, inner=side["s"])
    for out_f32 in (True, False):
        for drop in (True, False):
            what = "cfg %d out %s dropout %s" % (cfg, "fp32" if out_f32 else "bf16", drop)
            out = _canvas(M, N, N + 8, torch.float32 if out_f32 else torch.bfloat16)
            kw = dict(p_drop=P_DROP, site=DROP_SITE, seed=DROP_SEED) if drop else {}
            ops.gemm(A, B, M, N, K, lda=K + 16, ldb=K + 8, out=out, ldc=N + 8, bias=side["bias"].float(), addend=s, ld_add=N + 16,
                     ln_addend=ln, c_cached=out_f32, tile=cfg, **kw)
            torch.cuda.synchronize()
            dk = dict(keep=side["keep"], drop_scale=1.0 / (1.0 - P_DROP)) if drop else {}
            r = GR.epilogue(acc, bias=side["bias"], addend=side["ln"], out="f32" if out_f32 else "bf16", **dk)
            g, e = out[:M, :N].double(), r["y"].to(out.device)
            bad = g != e
            assert not bool(bad.any()), "%s: %d of %d elements differ from the fp64 result, first at %s (got %r, fp64 %r)" % (
                what, int(bad.sum()), bad.numel(), tuple(int(i) for i in bad.nonzero()[0]), float(g[bad][0]), float(e[bad][0]))
            _assert_canary(out, M, N, what)
            assert bool((s[:M, :N].double() == side["s"]).all()), what + ": the addend rows were written"


# ------------------------------------------------------------------------------------------------ engine
def _tensors(x, out):
    if torch.is_tensor(x):
        out.append(x.detach().clone())
    elif isinstance(x, (list, tuple)):
        for v in x:
            _tensors(v, out)
    elif x is not None:
        out.append(torch.tensor(float(x)))


def _engine_run(cfg, batch, ln_addend, train, dropout):
    params = dict(CFG.default_params(categories=9, residual_fp32=True), device=torch.device("cuda:0"))
    model = VisualDialogEncoder(dict(params, quiet_init=True), config=cfg)
    core = model.bert_pretrained
    core.cls_dropout = 0.1 if dropout else 0.0
    S.seeded_fill_(model.state_dict(), base_seed=7)
    core._invalidate_shadow()
    core.ln_addend = ln_addend
    model.train(train)
    assert core.residual_fp32
    out = step_forward(model, batch, params)
    eng = core._engine
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    taps = {}
    names = ["emb.t", "emb.v", "seq_t", "seq_v"]
    for i in range(16):
        names += ["%s%d.%s" % (k, i, sfx) for k in "tvc" for sfx in ("t", "v", "qkv", "qkv1", "qkv2")]
    for name in names:
        try:
            taps[name] = eng.tap(name, B, T, V).clone()
        except RuntimeError:
            pass
    outs = []
    _tensors(out, outs)
    grads = None
    if train:
        out[0].backward()
        grads = core.flat_grads.clone()
    torch.cuda.synchronize()
    ws = eng.workspace.numel()
    return outs, taps, grads, ws


def _engine_cfg(which):
    return CFG.tiny_config() if which == "tiny" else CFG.vilbert_config(v_feature_size=2048)


@pytest.mark.parametrize("dropout", [True, False], ids=["dropout", "nodropout"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_engine_ln_addend_route_equals_the_two_output_route(which, train, dropout):
    cfg = _engine_cfg(which)
    if dropout and which == "tiny":          # the tiny fixture config has its dropout probabilities at 0
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.1
        cfg.v_hidden_dropout_prob = cfg.v_attention_probs_dropout_prob = 0.1
    elif not dropout:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
        cfg.v_hidden_dropout_prob = cfg.v_attention_probs_dropout_prob = 0.0
    batch = S.make_batch(2, 5, 7, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=5)
    o0, t0, g0, ws0 = _engine_run(cfg, batch, False, train, dropout)
    o1, t1, g1, ws1 = _engine_run(cfg, batch, True, train, dropout)
    assert ws1 < ws0, "the default route plans no fp32 LayerNorm outputs"
    assert len(t0) >= 8 and t0.keys() == t1.keys()
    assert len(o0) == len(o1) and len(o0) >= 4
    for i, (a, b) in enumerate(zip(o0, o1)):
        assert a.shape == b.shape and torch.equal(a.float(), b.float()), "step output %d" % i
        assert bool(torch.isfinite(a.float()).all()), "step output %d" % i
    bad = [k for k in t0 if not torch.equal(_bits(t0[k]), _bits(t1[k]))]
    assert not bad, bad
    if train:
        assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
        assert torch.equal(_bits(g0), _bits(g1))
