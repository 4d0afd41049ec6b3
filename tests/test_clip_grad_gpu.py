"""Global-norm gradient clipping on the flat gradient buffers (-m gpu): crct_grad_sumsq / crct_grad_norm_finalize /
crct_scale_runs through the C ABI, and FusedAdamW.clip_grad_norm_ on top of them.

The tolerance on a norm is DERIVED, not measured.  All summands are non-negative, and a chunk's fp32 sum goes through at most 64
dependent fp32 roundings (the kernel's tree has 15): relative error <= 64 * 2^-24 = 3.8e-6.  The fp64 combine of the chunk sums adds
nothing visible, the square root halves the bound, one fp32 rounding of the result adds 6e-8:

    |norm - ref| <= 4e-6 * ref        against a float64 reference over the same stored values.

Everything else is exact: max |g|, the product of crct_scale_runs, results over repeated runs and over the launch width, a
power-of-two GradScaler factor, and the three ways a coefficient reaches the update (deferred, in place, overlapped launches).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import ops                               # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import GOLDEN                         # noqa: E402

DEV = torch.device("cuda:0")
NORM_RTOL = 4e-6
INF, NAN = float("inf"), float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ kernel level
SIZES = [4096 * 3 + 17, 64, 5000, 768, 1, 3 * 1024 * 1024 + 1037]      # the layout of test_adamw_matches_torch + one large tensor
SCALES = [1e-6, 1e-3, 1.0, 30.0, 1e3, 1e-2]
PAD = 1e30


class Flat(object):
    """A synthetic flat gradient buffer: tensors at 64-element aligned offsets, PAD (1e30) in the gaps -- which nothing may read."""

    def __init__(self, seed=0):
        self.offs, top = [], 0
        for s in SIZES:
            self.offs.append(top)
            top += (s + 63) // 64 * 64
        self.top = top
        g = torch.Generator().manual_seed(seed)
        host = torch.full((top,), PAD, dtype=torch.float32)
        self.used = torch.zeros(top, dtype=torch.bool)
        for o, s, sc in zip(self.offs, SIZES, SCALES):
            host[o:o + s] = torch.randn(s, generator=g) * sc
            self.used[o:o + s] = True
        self.host = host
        blk_seg, blk_off = ops.adamw_plan(SIZES)
        d = lambda t, dt: torch.as_tensor(t, dtype=dt).to(DEV)   # noqa: E731
        self.seg_off, self.seg_len = d(self.offs, torch.int64), d(SIZES, torch.int64)
        self.blk_seg, self.blk_off = blk_seg.to(DEV), blk_off.to(DEV)
        self.n_blk, self.n_seg = int(blk_seg.numel()), len(SIZES)

    def sumsq(self, g32, g16, kind=0, max_workgroups=0):
        """crct_grad_sumsq with BOTH buffers handed over as given (the wrapper in crct.ops passes only the one it reads)."""
        partials = torch.full((self.n_blk,), NAN, dtype=torch.float32, device=DEV)
        L.check(L.load().crct_grad_sumsq(L.ptr(g32), L.ptr(g16), self.seg_off.data_ptr(), self.seg_len.data_ptr(), self.blk_seg.data_ptr(),
                                         self.blk_off.data_ptr(), self.n_blk, partials.data_ptr(), kind, max_workgroups, L.current_stream()),
                "grad_sumsq")
        return partials

    def norms(self, g32, g16, kind=0, max_norm=INF, max_workgroups=0, grad_scale=None, mul=None):
        partials = self.sumsq(g32, g16, kind, max_workgroups)
        out, per = ops.grad_norm_finalize(partials, self.blk_seg, self.n_seg, max_norm, norm_kind=kind, grad_scale=grad_scale, mul=mul)
        torch.cuda.synchronize()
        return partials, out, per

    def reference(self, values, kind=0):
        """float64 norms (total, per tensor) of ``values`` (host fp32 tensor holding the stored values)."""
        v = values.double().numpy()
        if kind:
            per = np.array([np.abs(v[o:o + s]).max() for o, s in zip(self.offs, SIZES)])
            return per.max(), per
        per = np.array([np.sqrt(np.sum(v[o:o + s] ** 2)) for o, s in zip(self.offs, SIZES)])
        return np.sqrt(np.sum(per ** 2)), per


def sources(flat, host=None):
    """(name, g_f32, g_bf16, the values the kernel must see) for the fp32 source and for the bf16 source beside a NaN fp32 buffer."""
    host = flat.host if host is None else host
    h16 = host.to(torch.bfloat16)
    return [("fp32", host.to(DEV), None, host),
            ("bf16", torch.full((flat.top,), NAN, dtype=torch.float32, device=DEV), h16.to(DEV), h16.float())]


def test_norms_against_float64():
    flat = Flat()
    for name, g32, g16, values in sources(flat):
        _, out, per = flat.norms(g32, g16, kind=0)
        ref, ref_per = flat.reference(values, 0)
        got, got_per = float(out[0]), per.double().cpu().numpy()
        print("%s: norm %.9g ref %.9g rel %.3g; per-tensor rel max %.3g" % (name, got, ref, abs(got - ref) / ref,
                                                                          float(np.max(np.abs(got_per - ref_per) / ref_per))))
        assert abs(got - ref) <= NORM_RTOL * ref, name
        assert np.all(np.abs(got_per - ref_per) <= NORM_RTOL * ref_per), name
        assert float(out[1]) == 1.0                      # max_norm = inf never clips
        # max |g|: exact
        _, out, per = flat.norms(g32, g16, kind=1)
        ref, ref_per = flat.reference(values, 1)
        assert float(out[0]) == ref, name
        assert np.array_equal(per.double().cpu().numpy(), ref_per), name
        # the wrapper picks the source by dtype and gives the same bits
        src = g16 if g16 is not None else g32
        assert torch.equal(ops.grad_sumsq(src, flat.seg_off, flat.seg_len, flat.blk_seg, flat.blk_off), flat.sumsq(g32, g16))


def test_results_are_bit_reproducible_over_runs_and_launch_width():
    flat = Flat(seed=1)
    for name, g32, g16, _ in sources(flat):
        for kind in (0, 1):
            first = None
            for max_workgroups in (0, 0, 2, 7, 256, 256):
                res = flat.norms(g32, g16, kind=kind, max_norm=1.0, max_workgroups=max_workgroups)
                if first is None:
                    first = res
                for a, b in zip(first, res):
                    assert torch.equal(bits(a), bits(b)), (name, kind, max_workgroups)
    # fp32 and bf16 source holding the same values: the same tree, the same bits
    rounded = flat.host.to(torch.bfloat16)
    a = flat.sumsq(rounded.float().to(DEV), None)
    b = flat.sumsq(None, rounded.to(DEV))
    assert torch.equal(bits(a), bits(b))


def test_clip_coefficient_is_torchs_arithmetic():
    flat = Flat(seed=2)
    g32 = flat.host.to(DEV)
    _, out, _ = flat.norms(g32, None)
    norm = float(out[0])
    _, out, _ = flat.norms(g32, None, max_norm=2.0 * norm)
    assert float(out[1]) == 1.0
    _, out, _ = flat.norms(g32, None, max_norm=0.5 * norm)
    want = np.float32(0.5 * norm) / (np.float32(float(out[0])) + np.float32(1e-6))
    assert isinstance(want, np.float32)
    print("coefficient %.9g expected %.9g" % (float(out[1]), float(want)))
    assert abs(float(out[1]) - float(want)) <= 2.4e-7 * float(want)
    quarter = torch.tensor([0.25], device=DEV)
    _, out_mul, _ = flat.norms(g32, None, max_norm=0.5 * norm, mul=quarter)
    assert float(out_mul[1]) == float(out[1]) * 0.25 and float(out_mul[0]) == float(out[0])
    # one inf element: norm inf, coefficient 0; one NaN element: both NaN -- in both norm kinds, from both sources
    where = flat.offs[2] + 77
    for bad in (INF, NAN):
        host = flat.host.clone()
        host[where] = bad
        for name, s32, s16, _ in sources(flat, host):
            for kind in (0, 1):
                _, out, per = flat.norms(s32, s16, kind=kind, max_norm=1.0)
                if bad == INF:
                    assert float(out[0]) == INF and float(out[1]) == 0.0, (name, kind)
                    assert float(per[2]) == INF and bool(torch.isfinite(per[[0, 1, 3, 4, 5]]).all())
                else:
                    assert bool(torch.isnan(out).all()), (name, kind)
                    assert bool(torch.isnan(per[2])) and bool(torch.isfinite(per[[0, 1, 3, 4, 5]]).all())


def test_grad_scale_of_a_power_of_two_commutes():
    flat = Flat(seed=3)
    scale = torch.tensor([1024.0], device=DEV)
    scaled_host = flat.host * 1024.0
    for (name, g32, g16, _), (_, s32, s16, _) in zip(sources(flat), sources(flat, scaled_host)):
        for kind in (0, 1):
            _, out, per = flat.norms(g32, g16, kind=kind, max_norm=1.0)
            _, out_s, per_s = flat.norms(s32, s16, kind=kind, max_norm=1.0, grad_scale=scale)
            assert torch.equal(bits(out), bits(out_s)) and torch.equal(bits(per), bits(per_s)), (name, kind)


def test_scale_runs_is_one_product_per_element():
    flat = Flat(seed=4)
    g0 = flat.host.to(DEV)
    used = flat.used.to(DEV)
    for max_workgroups in (0, 7):
        coef = torch.tensor([0.37], device=DEV)
        g = g0.clone()
        ops.scale_runs(g, coef, flat.seg_off, flat.seg_len, flat.blk_seg, flat.blk_off, max_workgroups=max_workgroups)
        torch.cuda.synchronize()
        assert torch.equal(g[used], (g0 * coef)[used])
        assert torch.equal(bits(g[~used]), bits(g0[~used]))             # padding untouched
        one = torch.tensor([1.0], device=DEV)
        ops.scale_runs(g, one, flat.seg_off, flat.seg_len, flat.blk_seg, flat.blk_off, max_workgroups=max_workgroups)
        torch.cuda.synchronize()
        assert torch.equal(bits(g)[used], bits(g0 * coef)[used]) and torch.equal(bits(g[~used]), bits(g0[~used]))


# ------------------------------------------------------------------------------------------------ optimizer level
def build_model(cfg, params, weights=None, seed=7):
    params = dict(params, device=DEV)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    core.cls_dropout = 0.0
    sd = model.state_dict()
    if weights is not None:
        for k in sd:
            sd[k].copy_(torch.from_numpy(weights["w." + k[len("bert_pretrained."):].replace("cls.predictions.decoder.weight", "bert.embeddings.word_embeddings.weight")]))
    else:
        S.seeded_fill_(sd, base_seed=seed)
    core._invalidate_shadow()
    return model, params


class Tiny(object):
    """The tiny model and fixture of test_fused_adamw_matches_reference_steps_and_overlap_mode."""

    def __init__(self):
        self.zw = np.load(os.path.join(GOLDEN, "tiny_L1.npz"))
        self.cfg = C.tiny_config()
        self.base = C.default_params(categories=9, L1=True)
        self.batch = S.make_batch(3, 7, 5, self.cfg.v_feature_size, categories=9, vocab_size=self.cfg.vocab_size, seed=11)

    def fresh(self, overlap=False, launch_groups=0):
        from crct.optim import get_optimizer
        model, params = build_model(self.cfg, self.base, weights=self.zw)
        opt = get_optimizer(params, model)
        opt.overlap = overlap
        opt.launch_groups = launch_groups
        return model, params, model.bert_pretrained, opt

    def backward(self, model, params, core, it=0, scaler=None):
        core._calls = it
        loss = step_forward(model, self.batch, params)[0]
        (loss if scaler is None else scaler.scale(loss)).backward()


def norm64(opt, buf, kind=0):
    """float64 norm over the optimizer's tensors of the flat buffer ``buf`` (on the device)."""
    if kind:
        return max(float(buf[e.offset:e.offset + e.numel].double().abs().max()) for e in opt._segs)
    return float(torch.stack([buf[e.offset:e.offset + e.numel].double().pow(2).sum() for e in opt._segs]).sum().sqrt())


def state(core, opt):
    opt.synchronize()
    torch.cuda.synchronize()
    return [bits(core.flat_params).clone(), bits(opt._m).clone(), bits(opt._v).clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


class Exchanged(object):          # what the optimizer asks a FlatGradDDP for (test_adamw_reads_an_exchanged_bf16_gradient_buffer)
    world, last_exchange = 1, None

    def __init__(self):
        self.buf = None

    def grad_source(self):
        return self.buf


def test_clipped_step_matches_torch():
    t = Tiny()
    model, params, core, opt = t.fresh()
    t.backward(model, params, core)
    torch.cuda.synchronize()
    ref = norm64(opt, core.flat_grads)
    max_norm = 0.5 * ref
    byname = dict(core.named_parameters())
    ref_params = [byname[e.name].detach().float().cpu().clone().requires_grad_(True) for e in opt._segs]
    for rp, e in zip(ref_params, opt._segs):
        rp.grad = core.flat_grads[e.offset:e.offset + e.numel].view(e.shape).cpu().clone()
    g0 = opt.param_groups[0]
    groups = [{"params": [rp], "lr": opt.param_groups[opt._group_of[e.name]]["lr"], "weight_decay": opt.param_groups[opt._group_of[e.name]]["weight_decay"]}
              for rp, e in zip(ref_params, opt._segs)]
    ref_opt = torch.optim.AdamW(groups, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"])
    before = bits(core.flat_grads).clone()
    got = opt.clip_grad_norm_(max_norm)
    assert got.dim() == 0 and got.is_cuda
    assert torch.equal(bits(core.flat_grads), before)                   # deferred: .grad keeps the unclipped values
    per = opt.grad_norms()
    assert per.shape == (len(opt._segs),) and opt.grad_norm_names == [e.name for e in opt._segs]
    opt.step()
    opt.synchronize()
    torch.cuda.synchronize()
    print("norm %.9g ref %.9g rel %.3g" % (float(got), ref, abs(float(got) - ref) / ref))
    assert abs(float(got) - ref) <= NORM_RTOL * ref
    for e, n in zip(opt._segs, per.double().cpu().tolist()):
        r = float(core.flat_grads[e.offset:e.offset + e.numel].double().pow(2).sum().sqrt())
        assert abs(n - r) <= NORM_RTOL * r, e.name
    ref_norm = torch.nn.utils.clip_grad_norm_(ref_params, max_norm)
    assert abs(float(ref_norm) - ref) <= 1e-5 * ref
    ref_opt.step()
    for rp, e in zip(ref_params, opt._segs):
        assert torch.allclose(core.flat_params[e.offset:e.offset + e.numel].view(e.shape).cpu(), rp.detach(), rtol=1e-5, atol=1e-7), e.name
        # the first moment is (1 - beta1) x the CLIPPED gradient: 2 x off if the coefficient never reached the update.  Both
        # coefficients are within 5e-6 of the exact one (4e-6 + 2 ulp here, torch's fp32 norm there)
        assert torch.allclose(opt._m[e.offset:e.offset + e.numel].view(e.shape).cpu(), ref_opt.state[rp]["exp_avg"], rtol=1e-5, atol=1e-30), e.name


def test_coefficient_is_consumed_by_exactly_one_step():
    t = Tiny()
    runs = {}
    for route in ("deferred", "in_place"):
        model, params, core, opt = t.fresh()
        t.backward(model, params, core, 0)
        torch.cuda.synchronize()
        max_norm = 0.5 * norm64(opt, core.flat_grads)
        opt.clip_grad_norm_(max_norm, in_place=(route == "in_place"))
        opt.step()
        opt.zero_grad()
        first = state(core, opt)
        t.backward(model, params, core, 1)
        opt.step()                                  # no clip call: nothing of the first step's coefficient may be left
        opt.zero_grad()
        runs[route] = (first, state(core, opt))
    assert same(runs["deferred"][0], runs["in_place"][0])
    assert same(runs["deferred"][1], runs["in_place"][1])
    # zero_grad() between the clip call and the step drops the coefficient
    res = []
    for clip_then_clear in (True, False):
        model, params, core, opt = t.fresh()
        if clip_then_clear:
            t.backward(model, params, core, 0)
            torch.cuda.synchronize()
            opt.clip_grad_norm_(0.5 * norm64(opt, core.flat_grads))
            opt.zero_grad()
        t.backward(model, params, core, 0)
        opt.step()
        res.append(state(core, opt))
    assert same(res[0], res[1])
    assert not same(res[0], runs["deferred"][0])     # ... and the clipped first step is not the unclipped one


def test_the_routes_of_the_coefficient_agree_bit_for_bit():
    t = Tiny()
    max_norm = None
    res = {}
    routes = {"deferred": {}, "in_place": {}, "overlap": dict(overlap=True), "overlap_groups": dict(overlap=True, launch_groups=3),
              "never": {}, "above": {}, "deferred_x_inv_scale": {}, "in_place_x_inv_scale": {}}
    for route, kw in routes.items():
        model, params, core, opt = t.fresh(**kw)
        half = torch.tensor([0.5], device=DEV) if route.endswith("inv_scale") else None
        for it in range(2):
            t.backward(model, params, core, it)
            if max_norm is None:
                torch.cuda.synchronize()
                max_norm = 0.5 * norm64(opt, core.flat_grads)
            if route == "above":
                n = opt.clip_grad_norm_(1e9)
            elif route != "never":
                n = opt.clip_grad_norm_(max_norm, in_place=route.startswith("in_place"))
            if half is not None:
                opt.step(inv_scale=half)
            else:
                opt.step()
            opt.zero_grad()
        res[route] = state(core, opt)
        if route != "never":
            assert float(n) > 0.0
    for route in ("in_place", "overlap", "overlap_groups"):
        assert same(res["deferred"], res[route]), route
    assert same(res["never"], res["above"])
    assert not same(res["never"], res["deferred"])
    assert same(res["deferred_x_inv_scale"], res["in_place_x_inv_scale"])      # step(inv_scale=) x pending coefficient (0.5: exact)
    assert not same(res["deferred_x_inv_scale"], res["deferred"])


def test_refusals():
    t = Tiny()
    model, params, core, opt = t.fresh()
    t.backward(model, params, core)
    opt.set_early(True)
    try:
        with pytest.raises(RuntimeError, match="set_early"):
            opt.clip_grad_norm_(1.0)
    finally:
        opt.set_early(False)
    with pytest.raises(ValueError, match="norm_type"):
        opt.clip_grad_norm_(1.0, norm_type=3)
    fake = Exchanged()
    fake.buf, core._ddp = core.flat_grads.to(torch.bfloat16), fake
    try:
        with pytest.raises(ValueError, match="materialize_grads"):
            opt.clip_grad_norm_(1.0, in_place=True)
    finally:
        core._ddp = None
    # the infinity norm, and the module-level spelling through the model
    from crct.optim import clip_grad_norm_
    torch.cuda.synchronize()
    assert float(clip_grad_norm_(model, INF, norm_type=INF)) == norm64(opt, core.flat_grads, kind=1)
    assert float(clip_grad_norm_(opt, INF, norm_type="inf")) == norm64(opt, core.flat_grads, kind=1)
    core.flat_grads[opt._segs[3].offset] = INF
    with pytest.raises(RuntimeError, match="non-finite"):
        opt.clip_grad_norm_(1.0, error_if_nonfinite=True)
    assert opt._clip is None


def test_grad_scaler_composes_with_the_clip():
    """train.py:208-212 with the clip line between scaler.scale(loss).backward() and scaler.step(optimizer), no unscale_."""
    t = Tiny()
    max_norm = None
    final, norms = {}, {}
    for route in ("plain", "scaled", "scaled_poisoned"):
        model, params, core, opt = t.fresh()
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6) if route != "plain" else None
        norms[route] = []
        for it in range(3):
            t.backward(model, params, core, it, scaler)
            if max_norm is None:
                torch.cuda.synchronize()
                max_norm = 0.5 * norm64(opt, core.flat_grads)
            if route == "scaled_poisoned" and it == 1:
                core.flat_grads[5] = INF
                skipped_from = state(core, opt)
            torch.cuda.synchronize()
            ref = norm64(opt, core.flat_grads) / (float(scaler.get_scale()) if scaler is not None else 1.0)
            if scaler is None:
                n = opt.clip_grad_norm_(max_norm)
                opt.step()
            else:
                n = opt.clip_grad_norm_(max_norm, grad_scaler=scaler)
                scaler.step(opt)
                scaler.update()
            norms[route].append((float(n), ref))
            if route == "scaled_poisoned" and it == 1:
                assert same(skipped_from, state(core, opt))              # the step was skipped as a whole
            opt.zero_grad()
        torch.cuda.synchronize()
        final[route] = (core.flat_params.clone(), opt)
    for route in ("plain", "scaled"):
        for got, ref in norms[route]:                                    # the norm of the UNSCALED gradients
            print("%s: norm %.9g ref %.9g" % (route, got, ref))
            assert abs(got - ref) <= NORM_RTOL * ref, route
    assert torch.allclose(final["plain"][0], final["scaled"][0], rtol=0, atol=2e-7)
    assert norms["scaled_poisoned"][1][0] == INF
    assert int(final["scaled_poisoned"][1]._step_dev.item()) == 2
    assert int(final["scaled"][1]._step_dev.item()) == 3


@pytest.mark.parametrize("overlap", [False, True])
def test_clip_reads_the_exchanged_bf16_buffer(overlap):
    t = Tiny()
    res, max_norm = [], None
    for mode in ("fp32_of_rounded", "bf16_buffer"):
        model, params, core, opt = t.fresh(overlap=overlap)
        fake = Exchanged()
        for it in range(2):
            t.backward(model, params, core, it)
            g16 = core.flat_grads.to(torch.bfloat16)
            torch.cuda.synchronize()
            ref = norm64(opt, g16)
            if max_norm is None:
                max_norm = 0.5 * ref
            if mode == "bf16_buffer":
                fake.buf, core._ddp = g16, fake
                core.flat_grads.fill_(NAN)                # must not be read
            else:
                core.flat_grads.copy_(g16.float())
            n = opt.clip_grad_norm_(max_norm)
            opt.step()
            core._ddp = None
            opt.zero_grad()
            got = float(n)
            print("%s step %d: norm %.9g ref %.9g" % (mode, it, got, ref))
            assert np.isfinite(got) and abs(got - ref) <= NORM_RTOL * ref, (mode, it)
        res.append(state(core, opt))
    assert same(res[0], res[1])


def test_clip_through_a_real_bf16_exchange():
    """FlatGradDDP at world size 1 on the RCCL route, bf16 payload, this package's optimizer attached: the reduced Linear weight
    gradients live only in the communication buffer, their fp32 .grad views are NaN on purpose -- torch's clip_grad_norm_ returns
    NaN there, this one the norm of what the update consumes."""
    import torch.distributed as dist
    from crct.ddp import FlatGradDDP
    from crct.optim import clip_grad_norm_
    t = Tiny()
    model, params, core, opt = t.fresh()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    try:
        ddp = FlatGradDDP(model, bucket_mb=0.05, broadcast=False)
        ddp.force_exchange = True
        assert not ddp.materializes()
        t.backward(model, params, core)
        torch.cuda.synchronize()
        src = ddp.grad_source()
        assert src is not None and src.dtype == torch.bfloat16
        ref = norm64(opt, src)
        before = state(core, opt)
        n = clip_grad_norm_(ddp, 0.5 * ref)
        got = float(n)
        print("norm %.9g ref %.9g" % (got, ref))
        assert np.isfinite(got) and abs(got - ref) <= NORM_RTOL * ref
        with pytest.raises(ValueError, match="materialize_grads"):
            opt.clip_grad_norm_(0.5 * ref, in_place=True)
        n = clip_grad_norm_(ddp, 0.5 * ref)
        opt.step()
        after = state(core, opt)
        assert not same(before, after) and bool(torch.isfinite(core.flat_params).all())
        # the gap this closes
        grads = [p for p in core.parameters() if p.grad is not None]
        assert bool(torch.isnan(torch.nn.utils.clip_grad_norm_(grads, 0.5 * ref)))
    finally:
        core._ddp = None
        dist.destroy_process_group()


def test_full_size_norms_against_float64():
    """vilbert.json at BASELINE configs[1] (B 80, V 36, T 20): 238 M gradient elements in 524 tensors, up to 5723 chunks in one tensor
    -- where the summation depth would show."""
    from crct.optim import get_optimizer
    cfg = C.vilbert_config(v_feature_size=2048)
    model, params = build_model(cfg, C.default_params(), weights=None, seed=5)
    core = model.bert_pretrained
    opt = get_optimizer(params, model)
    batch = S.make_batch(80, 20, 36, 2048, seed=21)
    core._calls = 0
    step_forward(model, batch, params)[0].backward()
    n1 = opt.clip_grad_norm_(INF)
    per1 = opt.grad_norms()
    n2 = opt.clip_grad_norm_(INF)
    per2 = opt.grad_norms()
    torch.cuda.synchronize()
    assert len(opt._segs) == 524 and per1.shape == (524,) and per1 is not per2
    assert torch.equal(bits(n1.reshape(1)), bits(n2.reshape(1))) and torch.equal(bits(per1), bits(per2))
    sq = torch.stack([core.flat_grads[e.offset:e.offset + e.numel].double().pow(2).sum() for e in opt._segs])
    ref_per, ref = sq.sqrt(), float(sq.sum().sqrt())
    got = float(n1)
    rel = ((per1.double() - ref_per).abs() / ref_per.clamp_min(1e-300))
    print("norm %.9g ref %.9g rel %.3g; per-tensor rel max %.3g" % (got, ref, abs(got - ref) / ref, float(rel.max())))
    assert ref > 0.0 and abs(got - ref) <= NORM_RTOL * ref
    assert bool(((per1.double() - ref_per).abs() <= NORM_RTOL * ref_per).all())
