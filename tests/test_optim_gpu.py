"""The flat-buffer kernels that own the weights, per element against fp64 and bit for bit against host models (-m gpu): the AdamW update
(csrc/optim.hip) with its bf16 shadow, e4m3 shadow, transposed e4m3 shadow, amax, AMP state, bf16 gradient source and fused zeroing;
the fp8 scale machinery (crct_fp8_update_scales / _quantize_weights / _transpose_weights / _quantize_bf16) and the run-table movers
(crct_cast_*, crct_cast_runs_*, crct_zero_runs, crct_adamw_advance).  The yardstick is tests/optim_ref.py, proved on the CPU by
tests/test_optim_ref_cpu.py.

Every buffer is laid out as the model lays its own: segments at 64-element-aligned offsets with padding between them; the padding
holds a sentinel that must survive every launch.

Largest |got - fp64| / budget: each test prints its own (run with -s).  NOT YET MEASURED ON THE MI355X: no GPU could be had when this
file was written; it has only run against host stand-ins for the kernels, which proves its own logic and nothing about the kernels.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops, lib as L   # noqa: E402
import optim_ref as R             # noqa: E402

DEV = "cuda"
SENT = 7.0e33                     # fp32 padding value no result takes
SENT16 = 0x7B7B                   # bf16 padding bit pattern (1.3e36)
LANES = L.FP8_AMAX_LANES
SEG_LENS = (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 17)      # the scalar tail alone, a tail after vectors, chunk edges


def _bits(t):
    """bit patterns, for comparisons in which a NaN equals itself and -0 differs from +0"""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    bad = a != b
    assert not bool(bad.any()), "%s: %d elements differ in bits, first at %d (%#x against %#x)" % (
        what, int(bad.sum()), int(bad.nonzero()[0]), int(a[bad][0]) & 0xFFFFFFFF, int(b[bad][0]) & 0xFFFFFFFF)


def _q8_torch(x, scale, fmax=448.0, dtype=torch.float8_e4m3fn):
    """torch's conversion of the clamped fp32 product: what optim_ref.q8 spells out bit by bit (tests/test_optim_ref_cpu.py proves them equal)"""
    return (x.detach().cpu().float() * torch.tensor(np.float32(scale))).clamp(-fmax, fmax).to(dtype).view(torch.uint8)


class _Layout:
    """Segments at 64-aligned offsets with at least R.PAD padding elements between them, and the device tables of the update."""

    def __init__(self, lens, off=None):
        self.len = list(lens)
        if off is None:
            off, top = [], 0
            for n in self.len:
                top = (top + 63) // 64 * 64 + R.PAD
                off.append(top)
                top += n
            self.total = (top + 63) // 64 * 64 + R.PAD
        else:
            self.total = (max(o + n for o, n in zip(off, self.len)) + 63) // 64 * 64 + R.PAD
        self.off = list(off)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in zip(self.off, self.len):
            self.inside[o:o + n] = True
        bs, bo = ops.adamw_plan(self.len)
        self.seg_off, self.seg_len = torch.tensor(self.off, dtype=torch.int64, device=DEV), torch.tensor(self.len, dtype=torch.int64, device=DEV)
        self.blk_seg, self.blk_off = bs.to(DEV), bo.to(DEV)

    def spread(self, values):
        out = torch.zeros(self.total)
        for o, n, x in zip(self.off, self.len, values):
            out[o:o + n] = x
        return out

    def padded(self, x, fill=SENT):
        return torch.where(self.inside, x, torch.full((), fill, dtype=x.dtype))


class _State:
    """p, g, m, v, pb of one run on the device (padding = sentinel) with the per-segment lr / wd; step() launches the update once and
    holds every result to the fp64 reference made from the state the launch started from."""

    def __init__(self, lay, p, g, m, v, lr, wd):
        self.lay = lay
        self.p, self.m, self.v = (lay.padded(x).to(DEV) for x in (p, m, v))
        self.pb = torch.full((lay.total,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        self.lr, self.wd = lay.spread(lr), lay.spread(wd)
        self.seg_lr, self.seg_wd = torch.tensor(lr, dtype=torch.float32, device=DEV), torch.tensor(wd, dtype=torch.float32, device=DEV)

    def launch(self, g_dev, t, **kw):
        lay = self.lay
        ops.adamw_step(self.p, g_dev, self.m, self.v, lay.seg_off, lay.seg_len, self.seg_lr, self.seg_wd, lay.blk_seg, lay.blk_off, step=t,
                       p_bf16=self.pb, **kw)
        torch.cuda.synchronize()

    def step(self, t, g, what, worst, inv_scale=None, grad_scale=None, zero=False, mw=0, device_step=False, found_inf=None, fp8=None):
        lay = self.lay
        before = [x.cpu() for x in (self.p, self.m, self.v)]
        ref = R.reference(before[0], g, before[1], before[2], self.lr, self.wd, t, inv_scale=inv_scale, grad_scale=grad_scale,
                          device_step=device_step)
        g_dev = lay.padded(g).to(DEV)
        amp = {}
        if grad_scale is not None:
            amp["grad_scale"] = torch.tensor([grad_scale], device=DEV)
        if device_step:
            amp["step"] = torch.tensor([t], dtype=torch.int32, device=DEV)
        if found_inf is not None:
            amp["found_inf"] = torch.tensor([found_inf], device=DEV)
        self.launch(g_dev, 1 if device_step else t, inv_scale=None if inv_scale is None else torch.tensor([inv_scale], device=DEV),
                    amp=amp or None, zero_grads=zero, max_workgroups=mw, fp8=fp8)
        ins = lay.inside
        after = dict(p=self.p.cpu(), m=self.m.cpu(), v=self.v.cpu())
        for n in R.OUTPUTS:
            worst[n] = max(worst.get(n, 0.0), R.assert_within(after[n][ins], ref[n][ins], ref["budget"][n][ins], "%s, step %d: %s" % (what, t, n)))
            assert bool((after[n][~ins] == SENT).all()), "%s, step %d: padding of %s overwritten" % (what, t, n)
        pb = self.pb.cpu()
        _same_bits(pb[ins], after["p"][ins].to(torch.bfloat16), "%s, step %d: bf16 shadow" % (what, t))
        assert bool((pb.view(torch.int16)[~ins] == SENT16).all()), "%s, step %d: padding of the bf16 shadow overwritten" % (what, t)
        g_after = g_dev.cpu()
        assert bool((g_after[~ins] == SENT).all()), "%s, step %d: padding of g overwritten" % (what, t)
        if zero:
            _same_bits(g_after[ins], torch.zeros(int(ins.sum())), "%s, step %d: g after the fused zeroing" % (what, t))
        else:
            _same_bits(g_after[ins], g[ins], "%s, step %d: g (no zeroing asked for)" % (what, t))
        return after


@pytest.fixture(scope="module")
def layout():
    return _Layout(SEG_LENS)


def _family_state(lay, family):
    p, g, m, v = R.make_family(family, lay.total, seed=2)
    pairs = R.lr_wd_pairs()
    lr, wd = zip(*[pairs[i % len(pairs)] for i in range(len(lay.len))])
    return (p, g, m, v), list(lr), list(wd)


# host-step launch variants: max_workgroups 0 / 1 / 3, fused zeroing, inv_scale_dev alone, amp.grad_scale alone, both together
VARIANTS = (dict(mw=0), dict(mw=1, zero=True), dict(mw=3, inv_scale=0.37), dict(mw=0, grad_scale=1024.0),
            dict(mw=3, zero=True, inv_scale=0.37, grad_scale=3.0))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_adamw_three_steps_per_element_against_fp64(layout, family):
    """Three steps (the gradient grows with the step) of every launch variant, on the eight segment lengths: p', m', v' per element within
    the derived budget; pb == bf16(p') bit for bit; the padding of p, m, v, pb, g intact; g exactly 0 inside the segments when the
    zeroing is fused, untouched when not."""
    (p, g, m, v), lr, wd = _family_state(layout, family)
    worst = {}
    for var in VARIANTS:
        st = _State(layout, p, g, m, v, lr, wd)
        for t in (1, 2, 3):
            st.step(t, g * float(t), "%s %s" % (family, var), worst, **var)
    print("%-9s host step   " % family + " ".join("%s %.3f" % (n, worst[n]) for n in R.OUTPUTS))


@pytest.mark.parametrize("zero,mw", [(False, 0), (True, 3)])
def test_adamw_bf16_gradient_source_is_the_fp32_of_the_rounded_gradient(layout, zero, mw):
    """g_bf16 given and g filled with NaN: p, m, v, pb come out bit-equal to the run that reads fp32(bf16(g)) from g -- scalar tails
    included -- and g is only written (zeroed when asked, else left as it was); the bf16 buffer is never written."""
    (p, g, m, v), lr, wd = _family_state(layout, "init")
    g16 = g.to(torch.bfloat16)
    a, b = _State(layout, p, g, m, v, lr, wd), _State(layout, p, g, m, v, lr, wd)
    ga = layout.padded(g16.float()).to(DEV)
    gb = layout.padded(torch.full_like(g, float("nan"))).to(DEV)
    gb0 = gb.clone()
    g16_dev = torch.where(layout.inside, g16.view(torch.int16), torch.full((), SENT16, dtype=torch.int16)).to(DEV).view(torch.bfloat16)
    g16_0 = g16_dev.clone()
    inv = torch.tensor([0.37], device=DEV)
    a.launch(ga, 2, inv_scale=inv, zero_grads=zero, max_workgroups=mw)
    b.launch(gb, 2, inv_scale=inv, zero_grads=zero, max_workgroups=mw, g_bf16=g16_dev)
    for n in ("p", "m", "v", "pb"):
        _same_bits(getattr(b, n), getattr(a, n), "bf16 gradient source: " + n)
    _same_bits(g16_dev, g16_0, "the bf16 gradient buffer")
    want = torch.where(layout.inside, torch.zeros(()), gb0.cpu()) if zero else gb0
    _same_bits(gb, want, "g beside a bf16 source")


def test_device_step_bias_corrections(layout):
    """amp.step on the device (powf in fp32; 1 - 0.999^t cancels there) at t in R.T_DEVICE, found_inf absent and 0: within the budget with
    its powf term.  The isolating input (p = m = v = 0, wd = 0, eps tiny, g = 1) shows the bias-correction ratio alone; its error in units
    of U (w1 + w2 / 2) is the figure POWF_ULPS is set from (optim_ref.py), printed here."""
    (p, g, m, v), lr, wd = _family_state(layout, "init")
    worst = {}
    for i, t in enumerate(R.T_DEVICE):
        st = _State(layout, p, g, m, v, lr, wd)
        st.step(t, g, "device step t=%d" % t, worst, device_step=True, found_inf=(None, 0.0)[i % 2], mw=(0, 3)[i % 2],
                grad_scale=(None, 1024.0)[i % 2])
    print("init      device step " + " ".join("%s %.3f" % (n, worst[n]) for n in R.OUTPUTS))
    iso = R.isolating_case(layout.total)
    z = torch.zeros(layout.total)
    figures = []
    for t in R.T_DEVICE:
        st = _State(layout, z, iso["g"], z, z, [iso["lr"]] * len(layout.len), [0.0] * len(layout.len))
        step = torch.tensor([t], dtype=torch.int32, device=DEV)
        st.launch(layout.padded(iso["g"]).to(DEV), 1, eps=iso["eps"], amp=dict(step=step))
        ref = R.reference(z, iso["g"], z, z, iso["lr"], 0.0, t, eps=iso["eps"], device_step=True)
        got = st.p.cpu()[layout.inside].double()
        delta = float((got / ref["p"][layout.inside] - 1.0).abs().max())
        w = R.powf_weight(t)
        figures.append("t=%d: %.2f U%s" % (t, delta / R.U, ", powf %.3f" % (delta / (R.U * w)) if w >= 1.0 else ""))
        R.assert_within(st.p.cpu()[layout.inside], ref["p"][layout.inside], ref["budget"]["p"][layout.inside], "isolating input, t=%d" % t)
    print("bias-correction ratio through the kernel, |got / fp64 - 1|: " + "   ".join(figures))


def test_adamw_advance():
    step = torch.tensor([5], dtype=torch.int32, device=DEV)
    ops.adamw_advance(step)
    assert int(step) == 6
    ops.adamw_advance(step, torch.zeros(1, device=DEV))
    assert int(step) == 7
    ops.adamw_advance(step, torch.ones(1, device=DEV))
    assert int(step) == 7
    ops.adamw_advance(step, torch.tensor([float("nan")], device=DEV))      # the scaler's found_inf is a sum of flags: anything but 0 skips
    assert int(step) == 7


# ------------------------------------------------------------------------------------------- the fp8 shadow in the update
class _Shadow:
    """optim_ref.shadow_fixture on the device: the update's buffers and the CrctFp8Shadow tables."""

    def __init__(self):
        fx = self.fx = R.shadow_fixture()
        self.lay = _Layout(fx["len"], off=fx["off"])
        assert self.lay.total == fx["total"] and bool((self.lay.inside == fx["inside"]).all())
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)       # noqa: E731
        self.seg_slot, self.seg_in, self.seg_t_ld = i32(fx["slot"]), i32(fx["seg_in"]), i32(fx["t_ld"])
        self.seg_t_base = torch.tensor(fx["t_base"], dtype=torch.int64, device=DEV)

    def fresh(self, transposed=True):
        fx = self.fx
        st = _State(self.lay, fx["p"], fx["g"], fx["m"], fx["v"], fx["lr"], fx["wd"])
        st.q = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        st.qt = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        st.scale = torch.tensor(fx["scales"], device=DEV)
        st.amax = torch.zeros(fx["n_slots"] * LANES, device=DEV)
        st.amax[(fx["n_slots"] - 1) * LANES:] = 123.0                         # the slot no segment has
        st.f8 = dict(q=st.q, seg_slot=self.seg_slot, scale=st.scale, amax=st.amax)
        if transposed:
            st.f8.update(qt=st.qt, seg_in=self.seg_in, seg_t_base=self.seg_t_base, seg_t_ld=self.seg_t_ld)
        return st


@pytest.fixture(scope="module")
def shadow():
    return _Shadow()


def _check_shadow(fx, st, transposed, what):
    p1 = st.p.cpu()
    q, qt, amax = R.shadow_model(fx, p1, transposed=transposed)
    _same_bits(st.q, q, what + ": q (e4m3 shadow, sentinels between the tensors included)")
    _same_bits(st.qt, qt, what + ": qt (transposed shadow, sentinels included)")
    assert not bool(((st.q.cpu()[fx["inside"]] & 0x7F) == 0x7F).any()), what + ": a NaN byte in the shadow"
    words = st.amax.cpu().view(fx["n_slots"], LANES)
    for sl in range(fx["n_slots"] - 1):
        assert float(words[sl].max()) == float(amax[sl]), "%s: amax of slot %d is %r, max |p'| %r" % (what, sl, float(words[sl].max()), float(amax[sl]))
    assert bool((words[-1] == 123.0).all()), what + ": amax words of a slot no segment has were written"
    assert st.scale.cpu().tolist() == [float(np.float32(s)) for s in fx["scales"]], what + ": the update changed a scale"


@pytest.mark.parametrize("mw", [0, 1, 2, 3])
def test_adamw_fp8_shadow_bit_for_bit(shadow, mw):
    """One update over the shadow fixture (tile walk, one tile column, bands of a fused weight, a shadow without transposed copy,
    unshadowed segments in between; with max_workgroups 1 .. 3 a workgroup alternates plain and tile chunks and reuses its LDS tile):
    q, qt and amax bit for bit against the host model of the p' the kernel wrote, p' / m' / v' themselves within the fp64 budget."""
    fx = shadow.fx
    st = shadow.fresh()
    worst = {}
    st.step(1, fx["g"], "shadow fixture, max_workgroups %d" % mw, worst, mw=mw, fp8=st.f8)
    _check_shadow(fx, st, True, "max_workgroups %d" % mw)
    p1 = st.p.cpu()
    _same_bits(p1[fx["planted"]], fx["p"][fx["planted"]], "the planted ties / subnormals / signed zeros (p' = p)")
    for sl in (1, 4):                                    # the saturating slots really saturate
        segs = [i for i, s in enumerate(fx["slot"]) if s == sl]
        assert any(float(p1[fx["off"][i]:fx["off"][i] + fx["len"][i]].abs().max()) * fx["scales"][sl] > 448.0 for i in segs)


def test_adamw_fp8_shadow_without_transposed_copy(shadow):
    """qt = NULL with q set: the same q (plain chunks instead of the tile walk), qt never touched."""
    fx = shadow.fx
    a, b = shadow.fresh(), shadow.fresh(transposed=False)
    a.step(1, fx["g"], "with qt", {}, mw=2, fp8=a.f8)
    b.step(1, fx["g"], "without qt", {}, mw=2, fp8=b.f8)
    _check_shadow(fx, b, False, "qt = NULL")
    for n in ("p", "m", "v", "pb", "q"):
        _same_bits(getattr(b, n), getattr(a, n), "qt = NULL against qt set: " + n)


@pytest.mark.parametrize("zero", [False, True])
def test_found_inf_leaves_every_buffer_bit_identical(shadow, zero):
    """found_inf = 1 skips the step as a whole: p, m, v, pb, q, qt, amax, scale and g (also with the zeroing fused) keep their bits."""
    fx = shadow.fx
    st = shadow.fresh()
    g = shadow.lay.padded(fx["g"]).to(DEV)
    names = ("p", "m", "v", "pb", "q", "qt", "amax", "scale")
    before = {n: getattr(st, n).clone() for n in names}
    g0 = g.clone()
    amp = dict(found_inf=torch.ones(1, device=DEV), step=torch.tensor([3], dtype=torch.int32, device=DEV), grad_scale=torch.tensor([8.0], device=DEV))
    st.launch(g, 1, amp=amp, fp8=st.f8, zero_grads=zero, max_workgroups=2)
    for n in names:
        _same_bits(getattr(st, n), before[n], "found_inf = 1: " + n)
    _same_bits(g, g0, "found_inf = 1: g")
    assert int(amp["step"]) == 3


# ------------------------------------------------------------------------------------------- crct_fp8_update_scales
def _scale_case(n, seed):
    """n entries + 3 guard entries: entry i has its maximum only in lane 0 / 63 / 31 (i % 4 = 0 / 1 / 2) or is all zero (i % 4 = 3)"""
    g = torch.Generator().manual_seed(seed)
    amax = torch.rand((n + 3) * LANES, generator=g) * 0.01
    top = torch.exp(torch.rand(n + 3, generator=g) * 12 - 6) + 0.02
    for i in range(n + 3):
        w = amax[i * LANES:(i + 1) * LANES]
        if i % 4 == 3:
            w.zero_()
        else:
            w[::3] = 0.0                                   # zeros among the words
            w[(0, 63, 31)[i % 4]] = top[i]
    scale = torch.rand(n + 3, generator=g) + 5.0
    return scale, amax


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_fp8_update_scales(n):
    """scale == fl32(fmax / max of the entry's words) exactly, wherever the maximum lies in the wave; an all-zero entry keeps its scale;
    reset clears the words; skip_if != 0 leaves everything; fmax 0 acts as 448; nothing past n is touched."""
    for reset in (0, 1):
        for skip in (None, 0.0, 1.0):
            for fmax in (448.0, 57344.0, 0.0):
                scale0, amax0 = _scale_case(n, 10 * n + reset)
                what = "n=%d reset=%d skip_if=%r fmax=%g" % (n, reset, skip, fmax)
                scale, amax = scale0.clone().to(DEV), amax0.clone().to(DEV)
                ops.fp8_update_scales(scale, amax, n=n, reset=reset, skip_if=None if skip is None else torch.tensor([skip], device=DEV), fmax=fmax)
                want_s, want_a = scale0.clone(), amax0.clone()
                if not skip:
                    for i in range(n):
                        a = np.float32(amax0[i * LANES:(i + 1) * LANES].max())
                        if a > 0:
                            want_s[i] = float(np.float32(fmax if fmax > 0 else 448.0) / a)
                    if reset:
                        want_a[:n * LANES] = 0.0
                _same_bits(scale, want_s, what + ": scale")
                _same_bits(amax, want_a, what + ": amax words")


@pytest.mark.parametrize("reset", [0, 1])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_fp8_update_scales_non_finite_maximum(reset, bad):
    """An inf or NaN maximum carries no information about the tensor's range: the entry's scale stays as it was (fmax / inf = 0 would
    quantise every value to 0) and its words are cleared whatever `reset` says, so a running maximum cannot pin it.  The entries beside
    it are updated as usual."""
    n = 5
    scale0, amax0 = _scale_case(n, 77)
    amax0[1 * LANES + 63] = bad                            # beside finite words, in the last lane
    amax0[2 * LANES:3 * LANES] = bad                       # every word
    amax0[4 * LANES + 0] = bad
    scale, amax = scale0.clone().to(DEV), amax0.clone().to(DEV)
    ops.fp8_update_scales(scale, amax, n=n, reset=reset, fmax=57344.0)
    want_s, want_a = scale0.clone(), amax0.clone()
    want_s[0] = float(np.float32(57344.0) / np.float32(amax0[:LANES].max()))           # entry 3 is all zero: it keeps its scale too
    for i in (1, 2, 4):
        want_a[i * LANES:(i + 1) * LANES] = 0.0
    if reset:
        want_a[:n * LANES] = 0.0
    _same_bits(scale, want_s, "non-finite amax: scale")
    _same_bits(amax, want_a, "non-finite amax: amax words")


# ------------------------------------------------------------------------------------------- crct_fp8_quantize_weights
def test_fp8_quantize_weights_exact_scaling(shadow):
    """The start-up quantisation over the shadow fixture's segments (slot -1 mixed in, a fused weight sharing a slot): scale[slot] ==
    fl32(448 / max |w|), q == e4m3(clamp(w scale)) bit for bit with the maximal element at +-448; an all-zero tensor keeps its scale and
    gets zero bytes; a tensor holding an inf keeps its scale (no scale 0); skipped segments' bytes and unused slots are untouched."""
    fx, lay = shadow.fx, shadow.lay
    p = fx["p"].clone()
    zero_seg, inf_seg = 4, 5                               # W_c (slot 2) all zero, W_d (slot 3) holds an inf
    p[fx["off"][zero_seg]:fx["off"][zero_seg] + fx["len"][zero_seg]] = 0.0
    p[fx["off"][inf_seg] + 777] = float("-inf")
    prev = [5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]
    scale = torch.tensor(prev, device=DEV)
    amax = torch.full((fx["n_slots"] * LANES,), 3.0, device=DEV)
    q = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    ops.fp8_quantize_weights(lay.padded(p).to(DEV), q, lay.seg_off, lay.seg_len, shadow.seg_slot, lay.blk_seg, lay.blk_off, scale, amax)
    torch.cuda.synchronize()
    want_s = list(prev)
    for sl in (0, 1, 4, 5):
        mx = max(float(p[o:o + n].abs().max()) for o, n, s in zip(fx["off"], fx["len"], fx["slot"]) if s == sl)
        want_s[sl] = float(np.float32(448.0) / np.float32(mx))
    assert scale.cpu().tolist() == [float(np.float32(s)) for s in want_s], (scale.cpu().tolist(), want_s)
    want_q = torch.full((fx["total"],), R.SENTINEL_BYTE, dtype=torch.uint8)
    for o, n, sl in zip(fx["off"], fx["len"], fx["slot"]):
        if sl >= 0:
            want_q[o:o + n] = R.q8(p[o:o + n], want_s[sl])
    _same_bits(q, want_q, "quantize_weights: q")
    got = q.cpu()
    for sl in (0, 1, 4, 5):                                # the maximal element becomes +-448
        segs = [(o, n) for o, n, s in zip(fx["off"], fx["len"], fx["slot"]) if s == sl]
        assert max(int((got[o:o + n] & 0x7F).max()) for o, n in segs) == 0x7E
    assert bool((got[fx["off"][zero_seg]:fx["off"][zero_seg] + fx["len"][zero_seg]] == 0).all())
    assert int(got[fx["off"][inf_seg] + 777]) == 0xFE      # -inf saturates


def test_fp8_quantize_weights_grid_wrap():
    """More chunks than the launch has workgroups (2050 > 2048): the grid-stride loop reaches the last ones."""
    n = 2050 * 4096
    lay = _Layout([n, 8])
    g = torch.Generator().manual_seed(5)
    p = torch.randn(lay.total, generator=g) * 0.02
    scale = torch.ones(2, device=DEV)
    amax = torch.zeros(2 * LANES, device=DEV)
    q = torch.full((lay.total,), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    ops.fp8_quantize_weights(lay.padded(p).to(DEV), q, lay.seg_off, lay.seg_len, torch.tensor([0, -1], dtype=torch.int32, device=DEV),
                             lay.blk_seg, lay.blk_off, scale, amax)
    torch.cuda.synchronize()
    o = lay.off[0]
    s = float(np.float32(448.0) / np.float32(p[o:o + n].abs().max()))
    assert scale.cpu().tolist() == [s, 1.0]
    want = torch.full((lay.total,), R.SENTINEL_BYTE, dtype=torch.uint8)
    want[o:o + n] = _q8_torch(p[o:o + n], s)
    _same_bits(q, want, "quantize_weights over 2050 chunks")


# ------------------------------------------------------------------------------------------- crct_fp8_transpose_weights
@pytest.mark.parametrize("mw", [0, 1, 3])
def test_fp8_transpose_weights(mw):
    """Several weights in one launch, tile-aligned and ragged: qt is the exact transposition per weight of position-coded bytes, the
    sentinels between the weights stay."""
    shapes = [(16, 16), (48, 80), (64, 64), (80, 208), (192, 128)]
    offs, top = [], 0
    for o, i in shapes:
        top = (top + 63) // 64 * 64 + R.PAD
        offs.append(top)
        top += o * i
    total = top + R.PAD
    q = np.full(total, R.SENTINEL_BYTE, dtype=np.uint8)
    want = np.full(total, R.SENTINEL_BYTE, dtype=np.uint8)
    for k, (off, (o, i)) in enumerate(zip(offs, shapes)):
        r, c = np.meshgrid(np.arange(o), np.arange(i), indexing="ij")
        q[off:off + o * i] = ((r * 31 + c * 17 + k) % 251).astype(np.uint8).reshape(-1)
        R.transpose_bytes(q, want, off, o, i)
        assert (want[off:off + o * i].reshape(i, o) == q[off:off + o * i].reshape(o, i).T).all()
    qt = torch.full((total,), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    ops.fp8_transpose_weights(torch.from_numpy(q).to(DEV), qt, offs, [s[0] for s in shapes], [s[1] for s in shapes], max_workgroups=mw)
    _same_bits(qt, torch.from_numpy(want), "transpose_weights, max_workgroups %d" % mw)


# ------------------------------------------------------------------------------------------- crct_fp8_quantize_bf16
@pytest.mark.parametrize("n", [8, 8 * 255, 8 * 257, 2048 * 256 * 8 + 8])
@pytest.mark.parametrize("with_amax,with_inf", [(True, False), (True, True), (False, True)])
def test_fp8_quantize_bf16(n, with_amax, with_inf):
    """Bit-exact against the host model at a power-of-two scale (planted e4m3 ties, subnormals, values beyond +-448, +-inf saturating)
    and at 17; amax exact; the bytes behind n untouched.  The last n passes the launch's 2048 workgroups."""
    g = torch.Generator().manual_seed(n)
    for sc in (16.0, 17.0):
        x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 2)
        k = min(n, len(R.PLANTED))
        x[(torch.arange(k) * 37) % n] = torch.tensor(R.PLANTED[:k]) / 16.0
        if with_inf:
            x[n // 2], x[n - 1] = float("inf"), float("-inf")
        xb = x.to(torch.bfloat16)
        q = torch.full((n + 16,), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        amax = torch.zeros(LANES, device=DEV) if with_amax else None
        ops.fp8_quantize_bf16(xb.to(DEV), q, torch.tensor([sc], device=DEV), amax)
        want = torch.full((n + 16,), R.SENTINEL_BYTE, dtype=torch.uint8)
        want[:n] = R.q8(xb.float(), sc) if n <= 4096 else _q8_torch(xb.float(), sc)
        _same_bits(q, want, "quantize_bf16 n=%d scale=%g" % (n, sc))
        if with_amax:
            assert float(amax.max()) == float(xb.float().abs().max()), (n, sc, float(amax.max()), float(xb.float().abs().max()))


# ------------------------------------------------------------------------------------------- casts and runs
def _cast_probe(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8)
    special = torch.tensor([1.00390625, 1.01171875, -1.00390625, float("inf"), -float("inf"), float("nan"), 1e-40, -3e-39, 0.0, -0.0, 3.4e38,
                            1.0 + 2.0 ** -9, 2.0 ** -133, 1.5 * 2.0 ** -133])     # bf16 ties, infinities, NaN, fp32 subnormals, the bf16 overflow edge
    k = min(n, len(special))
    x[(torch.arange(k) * 5) % n] = special[:k]
    return x


def _same_or_both_nan(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want.float())
    assert bool((torch.isnan(got.float()) == nan).all()), what + ": NaN positions differ"
    _same_bits(torch.where(nan, torch.zeros((), dtype=got.dtype), got), torch.where(nan, torch.zeros((), dtype=want.dtype), want), what)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2051, 4096 * 256 * 8 + 5])
def test_casts_round_to_nearest_even_and_back(n):
    """crct_cast_f32_bf16 == torch's round-to-nearest-even, crct_cast_bf16_f32 exact, NaN compared as NaN; the elements behind n stay.
    The last n passes the launches' 4096 workgroups and leaves a 5-element tail."""
    x = _cast_probe(n, n)
    y = torch.full((n + 8,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ops.cast_bf16(x.to(DEV), out=y)
    _same_or_both_nan(y[:n], x.to(torch.bfloat16), "cast_f32_bf16 n=%d" % n)
    assert bool((y[n:].view(torch.int16) == SENT16).all())
    bits = torch.randint(-32768, 32768, (n,), generator=torch.Generator().manual_seed(n + 1), dtype=torch.int16)      # every kind of bf16 pattern
    k = min(n, 6)
    bits[:k] = torch.tensor([0x7F80, -128, 0x7FC0, 0x0001, -32768, 0x0080], dtype=torch.int16)[:k]                      # +inf, -inf, NaN, subnormal, -0, min normal
    xb = bits.view(torch.bfloat16)
    z = torch.full((n + 8,), SENT, device=DEV)
    ops.cast_f32(xb.to(DEV), out=z)
    _same_or_both_nan(z[:n], xb.float(), "cast_bf16_f32 n=%d" % n)
    assert bool((z[n:] == SENT).all())


@pytest.fixture(scope="module")
def runs():
    """Run table: every base mod 8 with every length of 1, 3, 7, 8, 9, 4096 + 5 (length 1 and 3 behind a longer head: head >= n), and one
    run of 2049 chunks + 3 at base mod 8 = 3 -- more chunks than the cast launches (2048) and the zeroing launch (1024) have workgroups."""
    off, lens, top = [], [], 16
    for r in range(8):
        for n in (1, 3, 7, 8, 9, 4096 + 5):
            top = (top + 3 + 7) // 8 * 8 + r
            off.append(top)
            lens.append(n)
            top += n
    top = (top + 3 + 7) // 8 * 8 + 3
    off.append(top)
    lens.append(2049 * 4096 + 3)
    total = top + lens[-1] + 16
    inside = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    bs, bo = ops.adamw_plan(lens)
    assert bs.numel() > 2048 and sorted(set(o % 8 for o in off)) == list(range(8))
    dev = lambda t, dt: torch.tensor(t, dtype=dt).to(DEV)      # noqa: E731
    return dict(off=dev(off, torch.int64), len=dev(lens, torch.int64), blk_seg=bs.to(DEV), blk_off=bo.to(DEV), inside=inside, total=total)


def test_cast_runs_both_directions(runs):
    """Head, vector and tail paths of both run casts at every base alignment, bit-exact, the destination untouched outside the runs."""
    ins, n = runs["inside"], runs["total"]
    x = _cast_probe(n, 3)
    y = torch.full((n,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ops.cast_runs(x.to(DEV), y, runs["off"], runs["len"], runs["blk_seg"], runs["blk_off"])
    want = torch.where(ins, x.to(torch.bfloat16).view(torch.int16), torch.full((), SENT16, dtype=torch.int16)).view(torch.bfloat16)
    _same_or_both_nan(y, want, "cast_runs_f32_bf16")
    xb = x.to(torch.bfloat16)
    z = torch.full((n,), SENT, device=DEV)
    ops.cast_runs(xb.to(DEV), z, runs["off"], runs["len"], runs["blk_seg"], runs["blk_off"])
    _same_or_both_nan(z, torch.where(ins, xb.float(), torch.full((), SENT)), "cast_runs_bf16_f32")


def test_zero_runs_on_a_non_finite_buffer(runs):
    """crct_zero_runs over the same table on a buffer of NaN and inf: +0 inside the runs, every bit outside kept."""
    ins, n = runs["inside"], runs["total"]
    g0 = torch.full((n,), float("nan"))
    g0[::3] = float("inf")
    g0[1::7] = -1.5
    g = g0.to(DEV)
    ops.zero_runs(g, runs["off"], runs["len"], runs["blk_seg"], runs["blk_off"])
    _same_bits(g, torch.where(ins, torch.zeros(()), g0), "zero_runs")
