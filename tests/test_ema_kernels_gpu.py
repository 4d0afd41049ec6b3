"""The weight average in the AdamW launch (csrc/optim.hip adamw_kernel<true>, through ops.adamw_step(..., ema=, ema_weight=)), per
element against fp64 and bit for bit against the launch without it (-m gpu).  The yardstick is tests/ema_ref.py, proved on the CPU by
tests/test_ema_ref_cpu.py: every e' is judged from THAT launch's own stored e and p', within the derived two-rounding budget.

Every buffer is laid out as the model lays its own: segments at 64-element-aligned offsets with padding between them; the padding holds
a sentinel that must survive every launch.  Each test prints its largest |got - fp64| / budget (run with -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import ema_ref as E               # noqa: E402
import optim_ref as R             # noqa: E402

DEV = "cuda"
SENT = 7.0e33                     # fp32 padding value no result takes
SENT16 = 0x7B7B                   # bf16 padding bit pattern
LANES = L.FP8_AMAX_LANES
INF, NAN = float("inf"), float("nan")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    bad = a != b
    assert not bool(bad.any()), "%s: %d elements differ in bits, first at %d (%#x against %#x)" % (
        what, int(bad.sum()), int(bad.nonzero()[0]), int(a[bad][0]) & 0xFFFFFFFF, int(b[bad][0]) & 0xFFFFFFFF)


class _Tables:
    """The device tables of the update over an ema_ref.Layout."""

    def __init__(self, lay):
        self.lay = lay
        bs, bo = ops.adamw_plan(lay.len)
        self.seg_off = torch.tensor(lay.off, dtype=torch.int64, device=DEV)
        self.seg_len = torch.tensor(lay.len, dtype=torch.int64, device=DEV)
        self.blk_seg, self.blk_off = bs.to(DEV), bo.to(DEV)
        self.blk_seg_host = bs

    def padded(self, x, fill=SENT):
        return torch.where(self.lay.inside, x, torch.full((), fill, dtype=x.dtype))


class _State:
    """p, m, v, pb, ema of one run on the device (padding = sentinel); launch() runs the update once, with the average when w is given."""
    NAMES = ("p", "m", "v", "pb", "ema")

    def __init__(self, tab, p, m, v, e, lr, wd):
        self.tab = tab
        self.p, self.m, self.v, self.ema = (tab.padded(x).to(DEV) for x in (p, m, v, e))
        self.pb = torch.full((tab.lay.total,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        self.seg_lr, self.seg_wd = torch.tensor(lr, dtype=torch.float32, device=DEV), torch.tensor(wd, dtype=torch.float32, device=DEV)

    def launch(self, g_dev, t, w=None, blocks=None, **kw):
        tab = self.tab
        bs, bo = (tab.blk_seg, tab.blk_off) if blocks is None else (tab.blk_seg[blocks[0]:blocks[1]], tab.blk_off[blocks[0]:blocks[1]])
        if w is not None:
            kw.update(ema=self.ema, ema_weight=float(w))
        ops.adamw_step(self.p, g_dev, self.m, self.v, tab.seg_off, tab.seg_len, self.seg_lr, self.seg_wd, bs, bo, step=t, p_bf16=self.pb, **kw)
        torch.cuda.synchronize()

    def snapshot(self):
        return {n: getattr(self, n).clone() for n in self.NAMES}


def _launch_kw(var, t, g, tab):
    """(g_dev, step argument, keywords) of launch variant `var` at step t with the host gradient g"""
    kw = dict(max_workgroups=var.get("mw", 0), zero_grads=var.get("zero", False))
    amp = {}
    if "inv_scale" in var:
        kw["inv_scale"] = torch.tensor([var["inv_scale"]], device=DEV)
    if "grad_scale" in var:
        amp["grad_scale"] = torch.tensor([var["grad_scale"]], device=DEV)
    if var.get("device_step"):
        amp["step"] = torch.tensor([t], dtype=torch.int32, device=DEV)
    if amp:
        kw["amp"] = amp
    if var.get("bf16"):
        g16 = g.to(torch.bfloat16)
        kw["g_bf16"] = torch.where(tab.lay.inside, g16.view(torch.int16), torch.full((), SENT16, dtype=torch.int16)).to(DEV).view(torch.bfloat16)
        g_dev = tab.padded(torch.full_like(g, NAN)).to(DEV)          # must not be read
    else:
        g_dev = tab.padded(g).to(DEV)
    return g_dev, (1 if var.get("device_step") else t), kw


def _check_average(tab, e_before, st, w, what, mask=None):
    """e' per element within the budget from the launch's own stored e and p' (inside the segments, or inside `mask`); the padding of
    the average intact; w = 0: every bit kept.  Returns the largest ratio."""
    ins = tab.lay.inside if mask is None else mask
    e_after, p_after = st.ema.cpu(), st.p.cpu()
    ref, budget = E.reference(e_before, p_after, w)
    worst = E.assert_within(e_after[ins], ref[ins], budget[ins], what)
    assert bool((e_after[~tab.lay.inside] == SENT).all()), what + ": padding of the average overwritten"
    if float(w) == 0.0:
        _same_bits(e_after, e_before, what + ": decay 1 must keep every bit of the average")
    return worst


@pytest.fixture(scope="module")
def tables():
    return _Tables(E.Layout())


# host step with max_workgroups 0 / 1 / 3, fused zeroing, inv_scale_dev, amp.grad_scale, the device step counter, the bf16 gradient source
VARIANTS = (dict(mw=0), dict(mw=1, zero=True), dict(mw=3, inv_scale=0.37), dict(mw=0, grad_scale=1024.0), dict(mw=3, device_step=True),
            dict(mw=1, bf16=True, zero=True))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_three_steps_per_element_against_fp64(tables, family):
    """Three steps (the gradient grows with the step) of every launch variant at every decay, on the eight segment lengths: e' per element
    within the derived budget from that launch's own e and p'; decay 1 keeps the average bit for bit; the padding of the average intact."""
    (p, g, m, v), lr, wd, e0 = E.family_inputs(family, tables.lay)
    worst = 0.0
    for var in VARIANTS:
        for decay in E.DECAYS:
            st = _State(tables, p, m, v, e0, lr, wd)
            w = E.weight(decay)
            for t in (1, 2, 3):
                before = st.ema.cpu()
                g_dev, step, kw = _launch_kw(var, t, g * float(t), tables)
                st.launch(g_dev, step, w=w, **kw)
                worst = max(worst, _check_average(tables, before, st, w, "%s %s decay %g step %d" % (family, var, decay, t)))
                assert bool(torch.isfinite(st.p.cpu()[tables.lay.inside]).all())
            if decay < 1.0:          # the average did move, in every segment
                e3 = st.ema.cpu()
                assert all(not torch.equal(e3[o:o + n], e0[o:o + n]) for o, n in zip(tables.lay.off, tables.lay.len))
    print("%-9s average: worst |got - fp64| / budget %.3f" % (family, worst))


@pytest.mark.parametrize("var", [dict(mw=0), dict(mw=3, zero=True, inv_scale=0.37), dict(mw=1, bf16=True), dict(mw=2, device_step=True, grad_scale=8.0)])
def test_the_average_is_an_observer(tables, var):
    """From identical states, a launch with the average and a launch without: p, m, v, pb and g bit-identical, padding included."""
    (p, g, m, v), lr, wd, e0 = E.family_inputs("init", tables.lay)
    a, b = _State(tables, p, m, v, e0, lr, wd), _State(tables, p, m, v, e0, lr, wd)
    ga, step, kwa = _launch_kw(var, 2, g, tables)
    gb, _, kwb = _launch_kw(var, 2, g, tables)
    a.launch(ga, step, w=None, **kwa)
    b.launch(gb, step, w=E.weight(0.999), **kwb)
    for n in ("p", "m", "v", "pb"):
        _same_bits(getattr(b, n), getattr(a, n), "observer %s: %s" % (var, n))
    _same_bits(gb, ga, "observer %s: g" % (var,))
    _same_bits(a.ema, tables.padded(e0), "the launch without the average wrote it")
    assert not torch.equal(b.ema, a.ema)


# ------------------------------------------------------------------------------------------- the tile walk and the fp8 shadows
class _Shadow:
    """optim_ref.shadow_fixture on the device: the update's buffers, the average and the CrctFp8Shadow tables."""

    def __init__(self):
        fx = self.fx = R.shadow_fixture()
        self.tab = _Tables(E.Layout(fx["len"], off=fx["off"]))
        assert self.tab.lay.total == fx["total"] and bool((self.tab.lay.inside == fx["inside"]).all())
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)       # noqa: E731
        self.seg_slot, self.seg_in, self.seg_t_ld = i32(fx["slot"]), i32(fx["seg_in"]), i32(fx["t_ld"])
        self.seg_t_base = torch.tensor(fx["t_base"], dtype=torch.int64, device=DEV)
        self.e0 = E.average_start(fx["total"], 9)

    def fresh(self):
        fx = self.fx
        st = _State(self.tab, fx["p"], fx["m"], fx["v"], self.e0, fx["lr"], fx["wd"])
        st.q = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        st.qt = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        st.scale = torch.tensor(fx["scales"], device=DEV)
        st.amax = torch.zeros(fx["n_slots"] * LANES, device=DEV)
        st.f8 = dict(q=st.q, seg_slot=self.seg_slot, scale=st.scale, amax=st.amax, qt=st.qt, seg_in=self.seg_in, seg_t_base=self.seg_t_base,
                     seg_t_ld=self.seg_t_ld)
        return st


@pytest.fixture(scope="module")
def shadow():
    return _Shadow()


@pytest.mark.parametrize("mw", [0, 1, 2, 3])
def test_tile_walk_and_fp8_shadows(shadow, mw):
    """The shadow fixture (transposed bands, bands of a fused QKV weight, a shadow without transposed copy, plain segments in between;
    with max_workgroups 1 .. 3 a workgroup alternates plain and tile chunks): e' per element within the budget -- the index of the
    average is the tile walk's own -- and p, m, v, pb, q, qt, the amax words and the scales bit-identical to the launch without it."""
    fx, tab = shadow.fx, shadow.tab
    a, b = shadow.fresh(), shadow.fresh()
    g = tab.padded(fx["g"]).to(DEV)
    w = E.weight(0.999)
    a.launch(g, 1, w=None, max_workgroups=mw, fp8=a.f8)
    b.launch(g, 1, w=w, max_workgroups=mw, fp8=b.f8)
    worst = _check_average(tab, tab.padded(shadow.e0), b, w, "shadow fixture, max_workgroups %d" % mw)
    for n in ("p", "m", "v", "pb", "q", "qt", "amax", "scale"):
        _same_bits(getattr(b, n), getattr(a, n), "shadow fixture, max_workgroups %d: %s" % (mw, n))
    # the host's wrong kernel (the average at the plain chunk index) is NOT what the device computed
    ref, budget = E.reference(shadow.e0, b.p.cpu(), w)
    wrong = E.emulate(shadow.e0, b.p.cpu(), w, mutate="plain_index", segs=E.shadow_segs(fx))
    assert bool(E.breaks(wrong, ref, budget)[fx["inside"]].any())
    print("tile walk, max_workgroups %d: worst ratio %.3f" % (mw, worst))


@pytest.mark.parametrize("zero", [False, True])
def test_found_inf_leaves_the_average_and_everything_else(shadow, zero):
    """found_inf = 1 skips the step as a whole: the average keeps its bits, as p, m, v, pb, q, qt, amax, scale and g do."""
    fx, tab = shadow.fx, shadow.tab
    st = shadow.fresh()
    g = tab.padded(fx["g"]).to(DEV)
    names = ("p", "m", "v", "pb", "ema", "q", "qt", "amax", "scale")
    before = {n: getattr(st, n).clone() for n in names}
    g0 = g.clone()
    amp = dict(found_inf=torch.ones(1, device=DEV), step=torch.tensor([3], dtype=torch.int32, device=DEV), grad_scale=torch.tensor([8.0], device=DEV))
    st.launch(g, 1, w=E.weight(0.9), amp=amp, fp8=st.f8, zero_grads=zero, max_workgroups=2)
    for n in names:
        _same_bits(getattr(st, n), before[n], "found_inf = 1: " + n)
    _same_bits(g, g0, "found_inf = 1: g")


def test_a_block_range_leaves_the_rest_of_the_average(tables):
    """A launch over a sub-range of the block table (FusedAdamW._launch(b0, b1)): the average inside the range's elements moves within
    the budget, outside it -- other segments, other chunks of the same segment -- every bit stays."""
    (p, g, m, v), lr, wd, e0 = E.family_inputs("init", tables.lay)
    lay = tables.lay
    n_blk = tables.blk_seg.numel()
    b0, b1 = 3, n_blk - 2                                    # drops the three shortest segments and the last two chunks of the longest
    touched = torch.zeros(lay.total, dtype=torch.bool)
    bs, bo = tables.blk_seg_host.tolist(), tables.blk_off.cpu().tolist()
    for b in range(b0, b1):
        o, n = lay.off[bs[b]] + bo[b], min(E.CHUNK, lay.len[bs[b]] - bo[b])
        touched[o:o + n] = True
    assert bool(touched.any()) and bool((lay.inside & ~touched).any())
    st = _State(tables, p, m, v, e0, lr, wd)
    before = st.snapshot()
    w = E.weight(0.9)
    st.launch(tables.padded(g).to(DEV), 1, w=w, blocks=(b0, b1), max_workgroups=3)
    _check_average(tables, before["ema"].cpu(), st, w, "block range", mask=touched)
    for n in _State.NAMES:
        _same_bits(getattr(st, n).cpu()[~touched], before[n].cpu()[~touched], "block range: %s outside the range" % n)
    assert not torch.equal(st.ema.cpu()[touched], before["ema"].cpu()[touched])


# ------------------------------------------------------------------------------------------- poisoned operands
def _planted(lay):
    """Elements away from chunk edges and on them: the sole element of the length-1 segment, the scalar tail of 4097, and in the longest
    segment its first element, a middle one, both sides of the first chunk edge, the first of a 16-byte group's neighbours and the last."""
    o1, o4097, olong = lay.off[0], lay.off[6], lay.off[7]
    return [o1, o4097 + 4096, olong, olong + 1001, olong + 4095, olong + 4096, olong + 2 * 4096 + 16]


@pytest.mark.parametrize("where", ["g", "p", "ema"])
@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_poisoned_operands_reach_their_own_element_only(tables, where, bad):
    """NaN / +-inf planted in g, p or the average: e' is non-finite exactly where the fp64 reference from the stored e and p' says so,
    which is the planted elements and nothing else; everywhere else it is within the budget."""
    (p, g, m, v), lr, wd, e0 = E.family_inputs("init", tables.lay)
    lay = tables.lay
    idx = _planted(lay)
    src = dict(g=g, p=p, ema=e0)[where].clone()
    src[idx] = bad
    st = _State(tables, src if where == "p" else p, m, v, src if where == "ema" else e0, lr, wd)
    before = st.ema.cpu()
    w = E.weight(0.999)
    st.launch(tables.padded(src if where == "g" else g).to(DEV), 1, w=w, max_workgroups=2)
    e_after, p_after = st.ema.cpu(), st.p.cpu()
    ref, budget = E.reference(before, p_after, w)
    planted = torch.zeros(lay.total, dtype=torch.bool)
    planted[idx] = True
    what = "%r planted in %s" % (bad, where)
    assert torch.equal(~torch.isfinite(ref) & lay.inside, planted), what + ": the reference is non-finite somewhere else"
    assert torch.equal(~torch.isfinite(e_after) & lay.inside, planted), what + ": non-finite values of the average are not the planted elements"
    ok = lay.inside & ~planted
    E.assert_within(e_after[ok], ref[ok], budget[ok], what)
    assert bool((e_after[~lay.inside] == SENT).all())


# ------------------------------------------------------------------------------------------- bad arguments
@pytest.mark.parametrize("w", [-0.1, 1.5, NAN])
def test_bad_ema_weight_launches_nothing(tables, w):
    (p, g, m, v), lr, wd, e0 = E.family_inputs("init", tables.lay)
    st = _State(tables, p, m, v, e0, lr, wd)
    before = st.snapshot()
    g_dev = tables.padded(g).to(DEV)
    g0 = g_dev.clone()
    with pytest.raises(RuntimeError, match="ema_weight"):
        st.launch(g_dev, 1, w=w, zero_grads=True)
    torch.cuda.synchronize()
    for n in _State.NAMES:
        _same_bits(getattr(st, n), before[n], "refused launch: " + n)
    _same_bits(g_dev, g0, "refused launch: g")
