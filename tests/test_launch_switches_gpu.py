"""The placement-only switches of the GEMM launches (-m gpu): crct_gemm_group_concat, crct_gemm_group_max_workgroups,
crct_gemm_group_target_workgroups / crct_engine_set_wgrad_workgroups and crct_gemm_fp8_scaled_mfma.  include/crct_hip.h promises the
same results for every value; bench.py flips all of them for A/B runs.  Kernel level: every problem of every group against its EXACT
result (integer operands, tests/gemm_ref.py: the expected bits come from fp64, never from another launch), the canaries round its output,
and the workgroup count in the launch log against the rules of csrc/tile_map.h, restated here in a few lines (tests/test_tile_map_cpu.py
walks those rules block by block on the CPU).  Engine level: a full-depth training step under every setting against the default one, loss
and flat gradients bit for bit, the log of the second backward showing that the switch took effect.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as GR                                          # noqa: E402
import test_kernels_gpu as TK                                  # noqa: E402
from crct import config as CFG, lib as L, ops                  # noqa: E402
from crct import synthetic as S                                # noqa: E402
from crct.step_adapter import forward as step_forward          # noqa: E402
from test_kernels_gpu import (DEV, SENT, _assert_bits, _assert_canary, _canvas, _f8, _group_problems, _logged, _q8,   # noqa: E402,F401
                              _wgrad_rowsum_case)
from test_step_gpu import build_model                          # noqa: E402

BM = BN = 128           # the tile of every grouped configuration (4, 9, 36, 37)
KIND_WGRAD = 2          # CRCT_KIND_WGRAD


# ------------------------------------------------------------------ the rules of csrc/tile_map.h, restated
def _tile_map(M, N):
    """make_tile_map for 128 x 128 tiles: (tiles_m, tiles_n, gn, rm, rn, blocks)."""
    tm, tn = -(-M // BM), -(-N // BN)
    best = None
    for gm in (1, 2, 4, 8):
        gn = 8 // gm
        rm, rn = -(-tm // gm), -(-tn // gn)
        cost = rm * BM + rn * BN + 4 * (rm * rn * 8 - tm * tn) * 16
        if best is None or cost < best[0]:
            best = (cost, gn, rm, rn)
    _, gn, rm, rn = best
    return tm, tn, gn, rm, rn, 8 * rm * rn


def _true_blocks(M, N):
    """Blocks of the map that map_tile gives a tile: must be tiles_m * tiles_n."""
    tm, tn, gn, rm, rn, blocks = _tile_map(M, N)
    n = 0
    for bid in range(blocks):
        x, j = bid & 7, bid >> 3
        hm, hn = min(rm, tm - (x // gn) * rm), min(rn, tn - (x % gn) * rn)
        n += hm > 0 and hn > 0 and j < hm * hn
    return n


def _group_total(shapes, concat):
    """Blocks a grouped launch over [(M, N)] walks: every problem's own map, or the concatenated tile list rounded up to the 8 XCDs."""
    if concat:
        return 8 * -(-sum(_tile_map(M, N)[0] * _tile_map(M, N)[1] for M, N in shapes) // 8)
    return sum(_tile_map(M, N)[5] for M, N in shapes)


def _group_grid(total, target, wgrad_bf16, cap):
    cap = (cap + 7) // 8 * 8 if cap > 0 else 0          # crct_gemm_group_max_workgroups keeps a multiple of 8
    if cap > 0:
        return min(cap, total)
    if not wgrad_bf16 or target <= 0 or total <= target:
        return total
    rounds = -(-total // target)
    return min((-(-total // rounds) + 7) // 8 * 8, total)


def _launches(fn):
    """fn() under the launch log, as test_kernels_gpu._logged, with the whole records (grid included)."""
    lib = L.load()
    lib.crct_launch_log_enable(1)
    try:
        out = fn()
    finally:
        recs = []
        for i in range(lib.crct_launch_log_count()):
            r = L.LaunchRec()
            lib.crct_launch_log_read(i, C.byref(r))
            recs.append(r)
        lib.crct_launch_log_enable(0)
    return out, recs


class _Switches(object):
    """concat / cap / library target / scaled MFMA for the length of a with block; always back to 0 / 0 / what it was / 1."""

    def __init__(self, concat=0, cap=0, target=None, scaled=1):
        self.v = (concat, cap, target, scaled)

    def __enter__(self):
        lib = L.load()
        concat, cap, target, scaled = self.v
        self.old_target = lib.crct_gemm_group_target_workgroups(0)
        try:
            lib.crct_gemm_group_target_workgroups(self.old_target if target is None else target)
            lib.crct_gemm_group_concat(concat)
            lib.crct_gemm_group_max_workgroups(cap)
            lib.crct_gemm_fp8_scaled_mfma(scaled)
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        lib = L.load()
        lib.crct_gemm_group_concat(0)
        lib.crct_gemm_group_max_workgroups(0)
        lib.crct_gemm_fp8_scaled_mfma(1)
        lib.crct_gemm_group_target_workgroups(self.old_target)
        return False


def test_the_restated_map_gives_every_tile_a_block():
    """The default case of the restated arithmetic against the number of true blocks, at the shapes of this file."""
    for M, N in [(104, 72), (120, 1032), (136, 200), (104, 136), (264, 200), (1024, 512), (776, 264), (3072, 768), (144, 208), (16, 16), (1600, 264)]:
        tm, tn, gn, rm, rn, blocks = _tile_map(M, N)
        assert _true_blocks(M, N) == tm * tn and blocks % 8 == 0 and blocks >= tm * tn, (M, N)


# ------------------------------------------------------------------ bf16 groups
def _wgrad_group(shapes, seed):
    """Weight-gradient problems as _group_problems("wgrad") builds them: accumulate, row sums on every other one."""
    probs, checks = [], []
    for i, (M, N, K) in enumerate(shapes):
        A, B, kw, acc, pre, rs_pre, rs_ref = _wgrad_rowsum_case(M, N, K, seed + 10 * i)
        out = _canvas(M, N, N + 8, torch.float32, inner=pre)
        d = dict(A=A, B=B, M=M, N=N, K=K, out=out, ldc=N + 8, accumulate=True, **kw)
        rs = None
        if i % 2 == 0:
            rs = torch.full((M + 8,), SENT, device=DEV)
            rs[:M] = rs_pre.float()
            d["rowsum_out"] = rs
        probs.append(d)
        checks.append((out, GR.f32(acc + pre), None, None, rs, rs_ref))
    return probs, checks


class _Group(object):
    """The problems of one grouped launch, built once: operands and exact results stay, every buffer a launch writes goes back to its
    first state (sentinels, accumulate-onto values) before the next launch, so a tile that is skipped cannot hide behind an earlier run."""

    def __init__(self, probs, checks):
        self.probs, self.checks = probs, checks
        self.first = [[None if b is None else b.clone() for b in (c[0], c[2], c[4])] for c in checks]
        self.shapes = [(d["M"], d["N"]) for d in probs]

    def run(self, tile):
        for (out, _, pre, _, rs, _), first in zip(self.checks, self.first):
            for b, f in zip((out, pre, rs), first):
                if b is not None:
                    b.copy_(f)
        for d in self.probs:
            d["tile"] = tile
        _, recs = _launches(lambda: ops.gemm_grouped(self.probs))
        return recs

    def check(self, what):
        for i, ((out, ref, pre, pre_ref, rs, rs_ref), d) in enumerate(zip(self.checks, self.probs)):
            w = "%s problem %d" % (what, i)
            M, N = d["M"], d["N"]
            _assert_bits(out[:M, :N], ref, w)
            _assert_canary(out, M, N, w)
            if pre is not None:
                _assert_bits(pre[:M, :N], pre_ref, w + ": preact_out")
                _assert_canary(pre, M, N, w + ": preact_out")
            if rs is not None:
                _assert_bits(rs[:M], rs_ref, w + ": rowsum_out")
                assert bool((rs[M:] == SENT).all()), w + ": rowsum_out written past M"


_WGRAD_GROUPS = {
    "eight": None,                                                     # the 8 problems of _group_problems("wgrad")
    "one_tile_beside_1x9": [(104, 72, 64), (120, 1032, 128)],          # 1 and 9 tiles: 8 + 16 blocks, 10 tiles -> 16 in concat mode
    "six_tiles": [(136, 200, 192), (104, 136, 64)],                    # 2 x 2 and 1 x 2 tiles: fewer than 8 in the whole group
}


@pytest.fixture(scope="module")
def wgrad_groups():
    out = {}
    for name, shapes in _WGRAD_GROUPS.items():
        out[name] = _Group(*(_group_problems("wgrad", seed=400) if shapes is None else _wgrad_group(shapes, seed=500)))
    return out


@pytest.mark.parametrize("name", list(_WGRAD_GROUPS))
@pytest.mark.parametrize("tile", (4, 9))
def test_bf16_weight_gradient_groups_under_every_placement(tile, name, wgrad_groups):
    """concat {0, 1} x cap {0, 1, 8, 24, 10000} x target {0, 7}: every problem bit for bit, canaries and row sums intact, and the logged
    grid the one tile_map.h's rules give (concat: the group walks 8 * ceil(tiles / 8) blocks)."""
    grp = wgrad_groups[name]
    tiles = sum(_tile_map(M, N)[0] * _tile_map(M, N)[1] for M, N in grp.shapes)
    assert _group_total(grp.shapes, 1) == 8 * math.ceil(tiles / 8)
    grids = set()
    for concat in (0, 1):
        for cap in (0, 1, 8, 24, 10000):
            for target in (0, 7):
                what = "wgrad %s cfg %d concat %d cap %d target %d" % (name, tile, concat, cap, target)
                with _Switches(concat=concat, cap=cap, target=target):
                    recs = grp.run(tile)
                assert [(r.cfg, r.split_k, r.n_problems, r.kind) for r in recs] == [(tile, 1, len(grp.probs), KIND_WGRAD)], what
                expect = _group_grid(_group_total(grp.shapes, concat), target, True, cap)
                assert recs[0].grid == expect, (what, recs[0].grid, expect)
                grids.add(recs[0].grid)
                grp.check(what)
    assert len(grids) >= 2, grids          # the switches moved the launch: more than one grid size was run (six_tiles: 16 and 8 blocks)


@pytest.mark.parametrize("mode", ["nt", "tb"])
@pytest.mark.parametrize("tile", (4, 9))
def test_forward_and_data_gradient_groups_ignore_concat_and_target_and_obey_the_cap(tile, mode):
    grp = _Group(*_group_problems(mode, seed=600 + tile))
    total = _group_total(grp.shapes, 0)
    seen = {}
    for concat, cap, target in ((0, 0, 0), (1, 0, 0), (0, 0, 7), (0, 8, 0), (1, 24, 7), (0, 10000, 0)):
        what = "%s cfg %d concat %d cap %d target %d" % (mode, tile, concat, cap, target)
        with _Switches(concat=concat, cap=cap, target=target):
            recs = grp.run(tile)
        assert [(r.cfg, r.split_k, r.n_problems) for r in recs] == [(tile, 1, len(grp.probs))], what
        seen[(concat, cap, target)] = recs[0].grid
        assert recs[0].grid == _group_grid(total, target, False, cap), (what, recs[0].grid, total)
        grp.check(what)
    assert seen[(1, 0, 0)] == seen[(0, 0, 0)] == seen[(0, 0, 7)] == total          # concat and the target: weight gradients only
    assert seen[(0, 8, 0)] == 8 and seen[(1, 24, 7)] == 24 and total > 24           # the cap changed the grid


# ------------------------------------------------------------------ fp8 weight-gradient groups
_F8_GROUP = ((144, 208), (16, 16), (768, 3072), (3072, 768), (272, 48), (64, 1040), (1024, 1024), (48, 336))      # test_gemm_fp8_weight_gradient_bit_for_bit


@pytest.fixture(scope="module")
def f8_group():
    R, sd, sx = 129, 4.0, 8.0
    sd_d, sx_d = torch.tensor([sd], device=DEV), torch.tensor([sx], device=DEV)
    probs, pres, refs = [], [], []
    for i, (N, K) in enumerate(_F8_GROUP):
        dq, xq = GR.ints((R, N), 8, 50 + i, "e5m2"), GR.ints((R, K), 16, 60 + i, "e4m3")
        pre = GR.unit_ints((N, K), 64, 70 + i, 1.0 / 32).to(DEV).float()
        probs.append((_f8(dq, "e5m2"), _f8(xq, "e4m3"), sd_d, sx_d, pre.clone()))
        pres.append(pre)
        refs.append(GR.f32(GR.ref_tt(dq.to(DEV), xq.to(DEV)) / (sd * sx) + pre.double()))
    GR.check_exact(R, 8, 16, 1 << 12, "e5m2")
    return probs, pres, refs


@pytest.mark.parametrize("tile", (36, 37))
def test_fp8_weight_gradient_group_under_every_placement(tile, f8_group):
    """concat {0, 1} x cap {0, 8, 40} x scaled MFMA {1, 0} on the 8-problem group with R = 129: bit for bit, the grid by the rules (an fp8
    group has no target: one workgroup per block unless capped)."""
    probs, pres, refs = f8_group
    lib = L.load()
    for concat in (0, 1):
        for cap in (0, 8, 40):
            for scaled in (1, 0):
                what = "fp8 wgrad group cfg %d concat %d cap %d scaled %d" % (tile, concat, cap, scaled)
                for p, pre in zip(probs, pres):
                    p[4].copy_(pre)
                with _Switches(concat=concat, cap=cap, target=7, scaled=scaled):
                    assert lib.crct_gemm_fp8_scaled_mfma(-1) == scaled
                    _, recs = _launches(lambda: ops.gemm_wgrad_fp8(probs, accumulate=True, tile=tile))
                assert [(r.cfg, r.split_k, r.n_problems) for r in recs] == [(tile, 1, 8)], what
                expect = _group_grid(_group_total(_F8_GROUP, concat), 7, False, cap)
                assert recs[0].grid == expect, (what, recs[0].grid, expect)
                for i, (p, ref) in enumerate(zip(probs, refs)):
                    _assert_bits(p[4], ref, "%s problem %d" % (what, i))
    assert lib.crct_gemm_fp8_scaled_mfma(-1) == 1


# ------------------------------------------------------------------ the plain fp8 MFMA (four 32-deep steps per 128-deep K tile)
def _plain(body, *args):
    """An existing test's body with crct_gemm_fp8_scaled_mfma(0), the switch read back round it."""
    lib = L.load()
    with _Switches(scaled=0):
        assert lib.crct_gemm_fp8_scaled_mfma(-1) == 0
        body(*args)
        assert lib.crct_gemm_fp8_scaled_mfma(-1) == 0
    assert lib.crct_gemm_fp8_scaled_mfma(-1) == 1


@pytest.mark.parametrize("M,N,K,cfg", [(257, 520, 384, 20), (300, 1000, 2048, 21), (130, 1032, 2048, 20), (1600, 768, 3072, 21)])
def test_plain_fp8_forward_bit_for_bit(M, N, K, cfg):
    """Exact operands: equal bits also prove that the four 32-deep steps pair the A and B fragments of the same K."""
    _plain(TK.test_gemm_fp8_forward_bit_for_bit, M, N, K, cfg)


@pytest.mark.parametrize("M,N,K,cfg", [(257, 264, 1024, 20), (300, 520, 2048, 21)])
def test_plain_fp8_data_gradient_bit_for_bit(M, N, K, cfg):
    _plain(TK.test_gemm_fp8_data_gradient_bit_for_bit, M, N, K, cfg)


@pytest.mark.parametrize("tile", (36, 37))
def test_plain_fp8_weight_gradient_bit_for_bit(tile):
    _plain(TK.test_gemm_fp8_weight_gradient_bit_for_bit, tile)          # single launches of five R, then the group of 8


def test_plain_fp8_weight_gradient_identity():
    _plain(TK.test_gemm_fp8_weight_gradient, 768, 768, 1024)            # R == N: dy = identity gives x itself, not its transpose


def _both_settings(launch):
    """launch() -> fp32 tensor, with the scaled and with the plain MFMA."""
    outs = []
    for scaled in (1, 0):
        with _Switches(scaled=scaled):
            outs.append(launch().clone())
    return outs


def _report(what, outs, ref):
    bound = 2e-3 * float(ref.abs().max())
    errs = [float((o.double() - ref).abs().max()) for o in outs]
    differ = int((outs[0].view(torch.int32) != outs[1].view(torch.int32)).sum())
    print("%s: max |err| scaled %.3e plain %.3e (bound %.3e); %d of %d output words differ between the two settings"
          % (what, errs[0], errs[1], bound, differ, outs[0].numel()))
    assert errs[0] <= bound and errs[1] <= bound, (what, errs, bound)


def test_plain_fp8_random_operands_against_fp64():
    """One random-operand case per kind against fp64 of the same dequantised operands, bound 2e-3 * max |ref| as in test_gemm_fp8_forward /
    _data_gradient / _weight_gradient, in both settings.  Printed, not asserted: how many fp32 output words differ between the scaled
    instruction and the four plain ones (the products are the same, the order of the fp32 additions need not be).
    Measured on MI355X: 0 of 307200 (forward), 0 of 307200 (data gradient), 0 of 16640 (weight gradient, configuration 36) and 0 of 16640
    (configuration 37) words differ; max |err| 1.9e-4 / 3.8e-7 / 4.1e-6 in either setting against bounds of 2.0e-2 / 3.9e-5 / 3.8e-4."""
    g = torch.Generator(device="cpu").manual_seed(77)
    # forward
    M, N, K = 300, 1024, 768
    x, w = torch.randn(M, K, generator=g) * 1.5, torch.randn(N, K, generator=g) * 0.05
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    sa, sb = 448.0 / float(x.abs().max()), 448.0 / float(w.abs().max())
    xq, wq = _q8(x, sa).to(DEV), _q8(w, sb).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    ref = (xq.double() / float(sa_d)) @ (wq.double() / float(sb_d)).t() + b.double()
    _report("forward 300x1024x768", _both_settings(lambda: ops.gemm_fp8(xq, wq, sa_d, sb_d, M, N, K, bias=b, out_f32=True)), ref)
    # data gradient: e5m2 x e4m3
    dy, wt = torch.randn(M, K, generator=g) * 3e-3, torch.randn(N, K, generator=g) * 0.05
    sa, sb = 57344.0 / float(dy.abs().max()), 448.0 / float(wt.abs().max())
    dyq, wq = (dy * sa).clamp(-57344, 57344).to(torch.float8_e5m2).to(DEV), _q8(wt, sb).to(DEV)
    sa_d, sb_d = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    ref = (dyq.double() / float(sa_d)) @ (wq.double() / float(sb_d)).t()
    _report("data gradient 300x1024x768", _both_settings(lambda: ops.gemm_fp8(dyq, wq, sa_d, sb_d, M, N, K, out_f32=True, a_bf8=True)), ref)
    # weight gradient: token-major e5m2 dy, e4m3 x
    R, N, K = 257, 208, 80
    dy, x = torch.randn(R, N, generator=g) * 3e-3, torch.randn(R, K, generator=g)
    s_dy, s_x = 57344.0 / float(dy.abs().max()), 448.0 / float(x.abs().max())
    dyq, xq = (dy * s_dy).clamp(-57344, 57344).to(torch.float8_e5m2).to(DEV), _q8(x, s_x).to(DEV)
    sd, sx = torch.tensor([s_dy], device=DEV), torch.tensor([s_x], device=DEV)
    ref = (dyq.double() / float(sd)).t() @ (xq.double() / float(sx))
    for tile in (36, 37):
        def launch():
            out = torch.full((N, K), 7.0, device=DEV)
            ops.gemm_wgrad_fp8([(dyq, xq, sd, sx, out)], accumulate=False, tile=tile)
            return out
        _report("weight gradient 257x208x80 cfg %d" % tile, _both_settings(launch), ref)


# ------------------------------------------------------------------ the step engine under every setting
# name -> (concat, cap, crct_engine_set_wgrad_workgroups arguments or None = the engine's default (96, 3000))
_ENGINE_SETTINGS = {"target0": (0, 0, (0, 3000)), "concat": (1, 0, None), "cap8": (0, 8, None), "cap40_concat": (1, 40, None),
                    "target8": (0, 0, (8, 3000)), "rows100": (0, 0, (96, 100)), "default_again": (0, 0, None)}


def _engine_run(fp8, concat, cap, wgs):
    """A fresh model (in fp8 mode the delayed scales move from pass to pass), the calibration pass, then the same two training passes:
    (loss, flat gradients, parameter table, grouped weight-gradient records of the second backward)."""
    cfg = CFG.vilbert_config(v_feature_size=2048)
    batch = S.make_batch(16, 20, 36, 2048, seed=5)
    model, params = build_model(cfg, CFG.default_params(fp8=fp8), weights=None, seed=3)
    core = model.bert_pretrained
    core.cls_dropout = 0.1
    with _Switches(concat=concat, cap=cap):
        step_forward(model, batch, params)          # creates the engine (fp8: the calibration pass)
        if wgs is not None:
            L.check(L.load().crct_engine_set_wgrad_workgroups(core._engine.handle, wgs[0], wgs[1]), "set_wgrad_workgroups")
        recs = None
        for _ in range(2):
            core.zero_flat_grads()
            core._calls = 0
            loss = step_forward(model, batch, params)[0]
            _, recs = _launches(loss.backward)
        torch.cuda.synchronize()
    groups = [r for r in recs if r.n_problems > 1 and r.kind == KIND_WGRAD]
    return float(loss.detach()), core.flat_grads.clone(), core.table, groups


@pytest.fixture(scope="module", params=[False, True], ids=["bf16", "fp8"])
def engine_base(request):
    """The default setting's run: what every other setting must reproduce bit for bit."""
    fp8 = request.param
    loss, grads, table, groups = _engine_run(fp8, 0, 0, None)
    assert torch.isfinite(grads).all() and groups
    return fp8, loss, grads, table, groups, {}


@pytest.mark.parametrize("name", list(_ENGINE_SETTINGS))
def test_engine_step_is_bit_identical_under_every_placement(name, engine_base):
    """Full-depth vilbert_config, B 16 x (20 text + 36 visual) rows, dropout on, one setting per case: loss and every used tensor of the
    flat gradients equal the default setting's bit for bit.  The grouped weight-gradient records of the second backward line up with the
    default run's, and their grids follow the setting: the group's full block count F with target 0 (and with the row threshold below the
    320 / 576 rows of this batch), group_grid(F, target) for the bf16 groups with a target (the fp8 groups have none), 8 under the cap of
    8, at most 40 under the cap of 40."""
    fp8, l0, g0, table, base, full_of = engine_base
    concat, cap, wgs = _ENGINE_SETTINGS[name]
    l1, g1, _, groups = _engine_run(fp8, concat, cap, wgs)
    assert l1 == l0, name
    bad = [e.name for e in table if e.used and not torch.equal(g0[e.offset:e.offset + e.numel], g1[e.offset:e.offset + e.numel])]
    assert not bad, (name, bad[:8])
    key = lambda r: (r.cfg, r.M, r.N, r.K, r.n_problems)      # noqa: E731
    assert [key(r) for r in groups] == [key(r) for r in base], name
    grids = [r.grid for r in groups]
    if name == "target0":                                        # F of every group: one workgroup per block
        assert all(f % 8 == 0 and f >= _tile_map(r.M, r.N)[5] for f, r in zip(grids, base))
        full_of["F"] = grids
        return
    if "F" not in full_of:                                       # (a case run on its own: the target-0 run has not been seen yet)
        full_of["F"] = [r.grid for r in _engine_run(fp8, 0, 0, (0, 3000))[3]]
    full = full_of["F"]
    bf16 = [r.cfg in (4, 9) for r in base]                       # (36 / 37: the fp8 groups)
    default = [_group_grid(f, 96, b, 0) for f, b in zip(full, bf16)]
    assert [r.grid for r in base] == default                     # the default run itself: the engine's target of 96 workgroups
    if not fp8:
        assert default != full                                   # groups above 96 blocks exist: the target shows
    if name == "rows100":
        assert grids == full                                     # the row threshold switches the policy off: as target 0
    elif name == "target8":
        assert grids == [_group_grid(f, 8, b, 0) for f, b in zip(full, bf16)] and (fp8 or grids != default)
    elif name == "default_again":
        assert grids == default
    elif name == "cap8":
        assert grids == [8] * len(base)                          # every group has at least 8 blocks
    elif name == "cap40_concat":
        for g, f, r in zip(grids, full, base):                   # min(40, 8 * ceil(tiles / 8)), tiles between problem 0's and F
            tiles0 = _tile_map(r.M, r.N)[0] * _tile_map(r.M, r.N)[1]
            assert g % 8 == 0 and min(40, 8 * math.ceil(tiles0 / 8)) <= g <= min(40, f), (g, f, r.M, r.N)
    else:
        assert name == "concat" and all(g % 8 == 0 and 8 <= g <= f for g, f in zip(grids, full))
