"""Host-only yardstick for the weight average the AdamW update keeps in its own launch (csrc/optim.hip: adamw_kernel<true>,
crct_adamw_step_ema): an fp64 reference with a derived per-element budget, an fp32 emulator with named mutants, and the inputs the
CPU and GPU tests share.  tests/test_ema_ref_cpu.py proves the yardstick, tests/test_ema_kernels_gpu.py and tests/test_ema_gpu.py
hold the kernel and the optimizer to it.

What the kernel computes per element it updates, from the fp32 weight p' it has just stored, the stored average e and w = 1 - decay:
    d  = fl(p' - e)
    e' = fl(w d + e)              one fused multiply-add
The reference is  ref = e + w (p' - e)  in fp64 from the STORED fp32 e, p', w.  Two roundings, each |fl(x) - x| <= U |x|
(U = 2^-24): e' - ref = w (p' - e) d1 + (ref + w (p' - e) d1) d2, so
    |e' - ref| <= U (w |p' - e| + |ref|) (1 + 4 U)
-- the factor (1 + 4 U) holds the second-order term (and the double rounding of an emulation that forms w d + e in fp64 first:
2^-53 relative against 4 U^2 = 2^-46).  Where ref is subnormal the final rounding is absolute, not relative: the smallest subnormal
is added there.  A difference p' - e in the subnormal range is exact.  Nothing is measured, nothing has a floor.

Inputs.  The update's own inputs are optim_ref's families on the eight segment lengths of tests/test_optim_gpu.py; what this module
chooses is what makes every mutant visible per element (asserted by tests/test_ema_ref_cpu.py, segment by segment and step by step):
  * lr 0.05 .. 0.2 (LR_WD): one step moves a weight by far more than U relative, also where v is large and g tiny;
  * the average starts at E0_SCALE x N(0, 1) = 2e-6, small against the weights and not zero: the budget U |ref| is then small
    against w |p' - p| down to w = 1e-4, and decay 1 has real bits to keep.
"""
import numpy as np
import torch

import optim_ref as R

U = R.U
SUBNORMAL = 2.0 ** -149
NORMAL_MIN = 2.0 ** -126
DECAYS = (0.9, 0.999, 0.9999, 1.0)
SEG_LENS = (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 17)      # the scalar tail alone, a tail after vectors, chunk edges
LR_WD = ((0.1, 0.01), (0.2, 0.0), (0.1, 0.01), (0.05, 0.01))
E0_SCALE = 2e-6
CHUNK = 4096
MUTANTS = ("old_p", "weights_swapped", "no_tail", "plain_index")


def weight(decay):
    """ema_weight as FusedAdamW forms it: the fp32 number nearest 1 - decay"""
    return np.float32(1.0 - float(decay))


# ------------------------------------------------------------------------------------------- reference and budget
def reference(e, p_new, w):
    """(ref, budget) in fp64 from the stored fp32 average, the stored fp32 new weight and the fp32 weight w."""
    E, P = e.detach().cpu().float().double(), p_new.detach().cpu().float().double()
    w = float(np.float32(w))
    diff = P - E
    ref = E + w * diff
    budget = U * (w * diff.abs() + ref.abs()) * (1.0 + 4.0 * U)
    budget = torch.where(ref.abs() < NORMAL_MIN, budget + SUBNORMAL, budget)
    return ref, budget


def assert_within(got, ref, budget, what):
    """Every element within its budget (both finite); names the first offender.  Returns the largest ratio."""
    return R.assert_within(got, ref, budget, what)


def breaks(got, ref, budget):
    """bool per element: outside the budget (a non-finite value counts as outside)"""
    g = got.detach().cpu().double()
    return ~((g - ref).abs() <= budget)


# ------------------------------------------------------------------------------------------- emulator and mutants
def _fma(w, d, e):
    """fl32(w d + e) for fp32 arrays: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    with np.errstate(all="ignore"):
        return (np.float64(w) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def tile_index(off, n, tin):
    """(tile-walk index, plain index) of every element the update visits in a segment [n / tin][tin] at `off` that keeps a transposed
    shadow: chunk c is the 64 x 64 tile (c / (tin / 64), c % (tin / 64)), element i of it lies at row i / 64, column i % 64."""
    k = np.arange(n, dtype=np.int64)
    c, i = k // CHUNK, k % CHUNK
    tiles_in = tin // 64
    tr, tc = c // tiles_in, c % tiles_in
    return off + tr * 64 * tin + tc * 64 + (i >> 6) * tin + (i & 63), off + k


def emulate(e, p_new, w, mutate=None, p_old=None, segs=None):
    """The kernel's two operations in fp32 over whole flat arrays (torch fp32 in, torch fp32 out).
    mutate (one of MUTANTS): the wrong kernels the budget must catch --
      old_p            averages the weight from before the update (needs p_old)
      weights_swapped  w and 1 - w exchanged
      no_tail          the scalar tail (the last len % 4 elements of a segment) is skipped     (needs segs)
      plain_index      a tile-walked tensor reads and writes its average at the plain chunk index (needs segs)
    segs: [(offset, length, tin)], tin > 0 for a segment the update walks tile by tile."""
    assert mutate is None or mutate in MUTANTS
    E = e.detach().cpu().float().numpy()
    P = (p_old if mutate == "old_p" else p_new).detach().cpu().float().numpy()
    w = np.float32(w)
    if mutate == "weights_swapped":
        w = np.float32(np.float32(1.0) - w)
    with np.errstate(all="ignore"):
        out = _fma(w, P - E, E)
    if mutate == "no_tail":
        for off, n, _ in segs:
            out[off + n - n % 4:off + n] = E[off + n - n % 4:off + n]
    if mutate == "plain_index":
        for off, n, tin in segs:
            if tin > 0:
                ti, pi = tile_index(off, n, tin)
                with np.errstate(all="ignore"):
                    out[pi] = _fma(w, P[ti] - E[pi], E[pi])
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------- layout and inputs
class Layout:
    """Segments at 64-aligned offsets with R.PAD padding elements in front of, between and behind them (host side only)."""

    def __init__(self, lens=SEG_LENS, off=None):
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

    def spread(self, values):
        out = torch.zeros(self.total)
        for o, n, x in zip(self.off, self.len, values):
            out[o:o + n] = x
        return out

    def segs(self, seg_in=None):
        return [(o, n, (seg_in[i] if seg_in else 0)) for i, (o, n) in enumerate(zip(self.off, self.len))]


def average_start(total, seed=0):
    """the average the tests start from: E0_SCALE N(0, 1), never exactly 0"""
    g = torch.Generator().manual_seed(4099 + seed)
    e = torch.randn(total, generator=g) * E0_SCALE
    return torch.where(e == 0, torch.full((), E0_SCALE), e)


def family_inputs(family, lay):
    """((p, g, m, v), lr per segment, wd per segment, e0) of one optim_ref family on the layout"""
    p, g, m, v = R.make_family(family, lay.total, seed=2)
    lr, wd = zip(*[LR_WD[i % len(LR_WD)] for i in range(len(lay.len))])
    return (p, g, m, v), list(lr), list(wd), average_start(lay.total, R.FAMILIES.index(family))


def shadow_segs(fx):
    return [(o, n, t) for o, n, t in zip(fx["off"], fx["len"], fx["seg_in"])]
