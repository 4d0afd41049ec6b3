"""Host-only yardstick for the flat-buffer kernels that own the weights (csrc/optim.hip: the AdamW update with its bf16 / e4m3 /
transposed e4m3 shadows; csrc/rowops.hip: the fp8 scale machinery and the casts): an fp64 reference of one AdamW step with a
per-element error budget, an fp32 emulator of the kernel's arithmetic with named mutants, bit-exact host models of every shadow the
update writes, and the inputs the CPU and GPU tests share.  tests/test_optim_ref_cpu.py proves the yardstick (the emulator stays
inside the budget, every mutant leaves it or differs in bits); tests/test_optim_gpu.py holds the kernels to it.

One step, as adamw_kernel computes it (every quantity fp32, `fl` one rounding):
    gsc    = inv_scale / grad_scale                     (either may be absent = 1)
    ga     = g gsc
    m'     = beta1 m + (1 - beta1) ga
    v'     = beta2 v + (1 - beta2) ga ga
    p'     = p (1 - lr wd)  -  lr inv_bc1 m' / (sqrt(v') inv_sqrt_bc2 + eps)
    inv_bc1 = 1 / (1 - beta1^t),  inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t)     host step: in double, then cast; device step: powf in fp32

The reference takes the hyper-parameters AS THE fp32 VALUES THE ABI RECEIVES (beta2 is the fp32 number nearest 0.999; 1 - beta2 is
then exact in fp32) and computes the above in fp64.  torch.optim.AdamW with double betas differs from it by (0.999 - fl32(0.999)) /
(1 - 0.999) = 1.3e-5 relative in v' (printed once by tests/test_optim_ref_cpu.py::test_reference_against_torch_adamw); nothing
here asserts that difference, tests/test_kernels_gpu.py::test_adamw_matches_torch keeps doing so at its own tolerance.

The budget is DERIVED from where the kernel rounds (U = 2^-24, the fp32 unit roundoff), never measured:
    m'   3 U (|beta1 m| + |(1 - beta1) ga|)                      two products and the sum      (+ n_g U |(1 - beta1) ga|)
    v'   3 U (beta2 v + (1 - beta2) ga^2)                        three roundings on either term (+ 2 n_g U (1 - beta2) ga^2)
         n_g = roundings behind ga: 0 without gradient scaling, 1 for the product g gsc, 1 more for the division by grad_scale
    p'   U (2 |p decay| + |p'|)    1 - lr wd rounded to fp32, the product p decay, the final subtraction -- each with the standard model
                                   |fl(x) - x| <= U |x|, also for 1 - lr wd just below 1 where half a step is U / 2
       + E_upd                     the update term upd = ss m' / den, ss = lr inv_bc1, den = sqrt(v') inv_sqrt_bc2 + eps:
         E_upd = |upd| (rel_ss + 2 U)                 ss carries rel_ss = rel(inv_bc1) + U; the product ss m' and the division
               + ss E_m / den                         the error m' already carries
               + |upd| E_den / den                    E_den = s (E_v / (2 v') + 2 U + rel(inv_sqrt_bc2)) + U den,  s = sqrt(v') inv_sqrt_bc2
         host step:   rel(inv_bc1) = rel(inv_sqrt_bc2) = U                              (computed in double, cast once)
         device step: rel(inv_bc1)      = U (c w1 + 2),           w1 = beta1^t / (1 - beta1^t)   powf, the cancelling subtraction, 1 / x
                      rel(inv_sqrt_bc2) = U ((c w2 + 1) / 2 + 2), w2 = beta2^t / (1 - beta2^t)   halved by the square root
         c = POWF_ULPS, the error of the device powf in units of U -- measured through the kernel, see the constant.
A budget of exactly 0 (p = g = m = v = 0) demands equality.  The budgets hold no absolute floor; they need normal fp32 numbers.
"""
import math
import os

import numpy as np
import torch

U = 2.0 ** -24
# Error of the device powf in units of 2^-24 relative: it cannot be derived here, it is measured on the MI355X through the kernel itself
# with the isolating input of `isolating_case` (p = m = v = 0, wd = 0, eps = 1e-30, g = 1: p' is the bias-correction ratio times
# -lr (1 - beta1) / sqrt(1 - beta2)).  tests/test_optim_gpu.py::test_device_step_bias_corrections prints, per t of T_DEVICE,
# |got / fp64 - 1| / (U (w1 + w2 / 2)) -- all of the error laid at powf's door -- and c is twice the largest, rounded up to an integer.
# NOT YET MEASURED ON THE GPU: 2 is a placeholder (numpy's fp32 power gives 0.004 / 0.22 / 0.30 / 0.08 at t = 1 / 2 / 3 / 10, which
# would make c = 1); the first GPU run of that test has to replace it and record its figures here.
POWF_ULPS = 2
T_DEVICE = (1, 2, 3, 10, 1000, 100000)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FAMILIES = ("p_zero", "init", "p_large", "sqrt_eps", "v_large")
MUTANTS = ("no_decay", "l2_decay", "eps_in_sqrt", "bc2_no_sqrt", "no_bc1", "beta1_for_v", "gsc_m_only", "grad_scale_multiplied")
SHADOW_MUTANTS = ("old_p", "amax_old_p", "truncate", "unclamped", "tile_swapped", "band_base")
OUTPUTS = ("p", "m", "v")


def f32(x):
    """the fp32 number nearest x, as a Python float: what a C float parameter receives"""
    return float(np.float32(x))


def lr_wd_pairs():
    """The (lr, wd) pairs the optimizer really uses (tests/golden/tiny_adamw3.npz: groups_lr_wd) plus (1e-3, 0.01) and (1e-3, 0)."""
    z = np.load(os.path.join(GOLDEN, "tiny_adamw3.npz"))
    pairs = sorted(set((float(a), float(b)) for a, b in z["groups_lr_wd"]))
    return pairs + [(1e-3, 0.01), (1e-3, 0.0)]


# ------------------------------------------------------------------------------------------- fp64 reference and budget
def reference(p, g, m, v, lr, wd, t, beta1=0.9, beta2=0.999, eps=1e-8, inv_scale=None, grad_scale=None, device_step=False,
              powf_ulps=None):
    """One step in fp64 on fp32 inputs (lr, wd: scalars or per-element tensors).  Returns dict(p, m, v, upd, budget=dict(p, m, v),
    terms=dict(...)): the new values, the update term, the per-element budgets of the module docstring and the magnitudes behind them."""
    c = POWF_ULPS if powf_ulps is None else powf_ulps
    b1, b2, ep = f32(beta1), f32(beta2), f32(eps)
    lr = torch.as_tensor(lr, dtype=torch.float32).double()
    wd = torch.as_tensor(wd, dtype=torch.float32).double()
    gs = (1.0 if inv_scale is None else f32(inv_scale)) / (1.0 if grad_scale is None else f32(grad_scale))
    n_g = int(inv_scale is not None or grad_scale is not None) + int(grad_scale is not None)
    P, G, M, V = (x.detach().cpu().double() for x in (p, g, m, v))
    ga = G * gs
    a_m, b_m = b1 * M, (1.0 - b1) * ga
    a_v, b_v = b2 * V, (1.0 - b2) * ga * ga
    m1, v1 = a_m + b_m, a_v + b_v
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    ss = lr / bc1
    isb2 = 1.0 / math.sqrt(bc2)
    s = v1.sqrt() * isb2
    den = s + ep
    upd = ss * m1 / den
    pd = P * (1.0 - lr * wd)
    p1 = pd - upd
    e_m = U * (3.0 * (a_m.abs() + b_m.abs()) + n_g * b_m.abs())
    e_v = U * (3.0 * (a_v + b_v) + 2.0 * n_g * b_v)
    if device_step:
        w1, w2 = b1 ** t / bc1, b2 ** t / bc2
        rel_ibc1, rel_isb2 = U * (c * w1 + 2.0), U * (0.5 * (c * w2 + 1.0) + 2.0)
    else:
        rel_ibc1 = rel_isb2 = U
    rel_ss = rel_ibc1 + U
    rel_v = torch.where(v1 > 0, e_v / v1.clamp_min(1e-300), torch.zeros(()).double())
    e_den = s * (0.5 * rel_v + 2.0 * U + rel_isb2) + U * den
    e_upd = upd.abs() * (rel_ss + 2.0 * U) + ss * e_m / den + upd.abs() * e_den / den
    e_p = U * (2.0 * pd.abs() + p1.abs()) + e_upd
    return dict(p=p1, m=m1, v=v1, upd=upd, budget=dict(p=e_p, m=e_m, v=e_v),
                terms=dict(decayed=pd.abs(), update=upd.abs(), m_terms=a_m.abs() + b_m.abs(), v_terms=a_v + b_v, den=den))


def ratio(got, ref, budget):
    """|got - ref| / budget per element (fp64); a zero budget demands equality (0 if equal, inf if not)."""
    err = (got.detach().cpu().double() - ref).abs()
    r = err / budget.clamp_min(1e-300)
    return torch.where(budget > 0, r, torch.where(err == 0, torch.zeros(()).double(), torch.full((), float("inf")).double()))


def assert_within(got, ref, budget, what):
    """Every element within its budget; names the first offender.  Returns the largest ratio."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    r = ratio(got, ref, budget)
    bad = r > 1.0
    assert not bool(bad.any()), "%s: %d elements beyond the budget, first at %d (got %r, fp64 %r, budget %r; worst ratio %.3f)" % (
        what, int(bad.sum()), int(bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]), float(budget[bad][0]), float(r.max()))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------- emulator
def grad_multiplier(inv_scale=None, grad_scale=None, multiplied=False):
    """gsc as the kernel forms it in fp32: (inv_scale or 1) / grad_scale"""
    gsc = np.float32(1.0 if inv_scale is None else inv_scale)
    if grad_scale is not None:
        gsc = np.float32(gsc * np.float32(grad_scale)) if multiplied else np.float32(gsc / np.float32(grad_scale))
    return gsc


def bias_corrections(beta1, beta2, t, device_step):
    """(inv_bc1, inv_sqrt_bc2) as fp32: in double from the fp32 betas and cast (host step), or in fp32 with powf (device step)."""
    b1, b2 = np.float32(beta1), np.float32(beta2)
    if device_step:
        st = np.float32(t)
        one = np.float32(1.0)
        return one / (one - np.power(b1, st, dtype=np.float32)), one / np.sqrt(one - np.power(b2, st, dtype=np.float32), dtype=np.float32)
    return np.float32(1.0 / (1.0 - float(b1) ** t)), np.float32(1.0 / math.sqrt(1.0 - float(b2) ** t))


def emulate(p, g, m, v, lr, wd, t, beta1=0.9, beta2=0.999, eps=1e-8, inv_scale=None, grad_scale=None, device_step=False, mutate=None):
    """adamw_kernel's arithmetic in torch fp32 on the CPU, operation by operation in the kernel's order (no fused multiply-adds: a
    contraction only removes roundings).  lr, wd: scalars or per-element fp32 tensors.  Returns fp32 p', m', v'.
    mutate (one of MUTANTS): the wrong kernels the budget must catch --
      no_decay               p is not decayed
      l2_decay               decay as coupled L2: g += wd p, no decoupled factor
      eps_in_sqrt            the denominator is sqrt(v' / bc2 + eps)
      bc2_no_sqrt            the second bias correction without its square root: sqrt(v') / bc2
      no_bc1                 the step size without 1 / bc1
      beta1_for_v            (1 - beta1) weighs g^2
      gsc_m_only             the gradient scale reaches m' but not v'
      grad_scale_multiplied  gsc = inv_scale * grad_scale"""
    assert mutate is None or mutate in MUTANTS
    T = lambda x: torch.as_tensor(np.float32(x) if not torch.is_tensor(x) else x, dtype=torch.float32)   # noqa: E731
    p, g, m, v = (x.detach().cpu().float() for x in (p, g, m, v))
    lr, wd = T(lr), T(wd)
    b1, b2, ep = T(beta1), T(beta2), T(eps)
    one = T(1.0)
    inv_bc1, isb2 = (T(x) for x in bias_corrections(beta1, beta2, t, device_step))
    gsc = T(grad_multiplier(inv_scale, grad_scale, multiplied=mutate == "grad_scale_multiplied"))
    decay = one - lr * wd
    ss = lr * (one if mutate == "no_bc1" else inv_bc1)
    ga = g * gsc
    if mutate in ("no_decay", "l2_decay"):
        decay = one
    if mutate == "l2_decay":
        ga = ga + wd * p
    pa = p * decay
    ma = b1 * m + (one - b1) * ga
    gv = g if mutate == "gsc_m_only" else ga
    va = b2 * v + ((one - (b1 if mutate == "beta1_for_v" else b2)) * gv) * gv
    if mutate == "eps_in_sqrt":
        den = torch.sqrt(va * isb2 * isb2 + ep)
    elif mutate == "bc2_no_sqrt":
        den = torch.sqrt(va) * (isb2 * isb2) + ep
    else:
        den = torch.sqrt(va) * isb2 + ep
    pa = pa - ss * ma / den
    return pa, ma, va


# ------------------------------------------------------------------------------------------- input families
def make_family(family, n, seed=0):
    """(p, g, m, v) fp32 CPU tensors [n].
    p_zero    p = 0 (p' = -update: the update term resolved to fp32 relative precision); g log-uniform 1e-8 .. 1e3 with signs and exact zeros
    init      p ~ 0.02 N(0, 1), the real initialisation; g as above; m, v a plausible history of such gradients
    p_large   |p| log-uniform 1 .. 30 (decay dominates); g as above
    sqrt_eps  p as init; |g| within a factor 2 of sqrt(eps) = 1e-4 and, for every fourth element, of eps = 1e-8; m = v = 0 for every other element
    v_large   v log-uniform 1e2 .. 1e6 with g tiny (1e-8 .. 1e-6) and m small"""
    assert family in FAMILIES
    gen = torch.Generator().manual_seed(7919 * seed + FAMILIES.index(family))
    rnd = lambda: torch.rand(n, generator=gen, dtype=torch.float64)         # noqa: E731
    sign = lambda: torch.where(rnd() < 0.5, -1.0, 1.0).double()             # noqa: E731
    g = sign() * torch.exp(math.log(1e-8) + rnd() * math.log(1e3 / 1e-8))
    g[rnd() < 0.05] = 0.0
    m = g * (0.2 + rnd()) * sign()
    v = g * g * (0.05 + 2.0 * rnd())
    p = 0.02 * torch.randn(n, generator=gen, dtype=torch.float64)
    if family == "p_zero":
        p = torch.zeros(n, dtype=torch.float64)
    elif family == "p_large":
        p = sign() * torch.exp(rnd() * math.log(30.0))
    elif family == "sqrt_eps":
        g = sign() * 1e-4 * (0.5 + 1.5 * rnd())
        g[::4] = g[::4] * 1e-4
        m = g * (0.2 + rnd()) * sign()
        v = g * g * (0.05 + 2.0 * rnd())
        m[1::2] = 0.0
        v[1::2] = 0.0
    elif family == "v_large":
        g = sign() * torch.exp(math.log(1e-8) + rnd() * math.log(1e2))
        v = torch.exp(math.log(1e2) + rnd() * math.log(1e4))
        m = 1e-3 * torch.randn(n, generator=gen, dtype=torch.float64)
    return p.float(), g.float(), m.float(), v.float()


def isolating_case(n=64):
    """p = m = v = 0, wd = 0, eps = 1e-30, g = 1: p' = -lr (1 - beta1) inv_bc1 / (sqrt(1 - beta2) inv_sqrt_bc2), the bias corrections alone."""
    z = torch.zeros(n)
    return dict(p=z.clone(), g=torch.ones(n), m=z.clone(), v=z.clone(), lr=1e-3, wd=0.0, eps=1e-30)


def powf_weight(t, beta1=0.9, beta2=0.999):
    """w1 + w2 / 2: how many units of the relative powf error reach p' of the isolating case"""
    b1, b2 = f32(beta1), f32(beta2)
    return b1 ** t / (1.0 - b1 ** t) + 0.5 * b2 ** t / (1.0 - b2 ** t)


# ------------------------------------------------------------------------------------------- bit-exact host models
def bf16_bits(x):
    """fp32 -> bf16, round to nearest even: int16 bit patterns"""
    return x.detach().cpu().float().to(torch.bfloat16).view(torch.int16)


def fp8_encode(x, kind="e4m3", mode="rne", clamp=True):
    """OCP fp8 bytes (uint8 tensor) of fp32 x as the kernels form them: saturate to +-fmax first (clamp), then round to nearest even.
    Written out bit by bit (no torch float8): tests/test_optim_ref_cpu.py checks it against torch's own conversion.
    kind 'e4m3' (fmax 448, bias 7, 3 mantissa bits) or 'e5m2' (fmax 57344, bias 15, 2 bits); mode 'rne' or 'trunc' (a mutant);
    clamp=False (a mutant): what lies beyond the largest finite number becomes the NaN byte 0x7F / 0xFF (e4m3) or inf 0x7C / 0xFC."""
    mb, bias, fmax = (3, 7, 448.0) if kind == "e4m3" else (2, 15, 57344.0)
    emin = 1 - bias
    a = x.detach().cpu().float().numpy().astype(np.float64)
    sign = np.signbit(a).astype(np.uint8) << 7
    a = np.abs(a)
    nan = np.isnan(a)
    if clamp:
        a = np.minimum(a, fmax)
    a = np.where(nan, 0.0, a)
    top_step = 2.0 ** (math.floor(math.log2(fmax)) - mb)          # spacing below fmax: what rounds past fmax + top_step / 2 is not finite
    if mode == "rne":                                              # the tie at fmax + top_step / 2 goes to the even mantissa: 448 (e4m3), inf (e5m2)
        over = a > fmax + top_step / 2 if kind == "e4m3" else a >= fmax + top_step / 2
    else:
        over = a >= fmax + top_step
    a = np.where(over | np.isinf(a), 0.0, a)
    e = np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -300))), emin)
    step = np.exp2(e - mb)
    k = a / step
    k = np.rint(k) if mode == "rne" else np.floor(k)               # np.rint rounds halves to even
    val = k * step
    fr, ex = np.frexp(np.maximum(val, 2.0 ** emin))                # val = fr 2^ex, fr in [0.5, 1)
    normal = val >= 2.0 ** emin
    byte = np.where(normal, ((ex - 1 + bias) << mb) + (fr * 2 ** (mb + 1) - 2 ** mb).astype(np.int64), k.astype(np.int64))
    byte = np.where(over | nan, 0x7F if kind == "e4m3" else 0x7C, byte)
    if kind == "e5m2":
        byte = np.where(nan, 0x7F, byte)
    return torch.from_numpy((byte.astype(np.uint8) | sign).astype(np.uint8))


def q8(x, scale, kind="e4m3", mode="rne", clamp=True):
    """The kernels' quantisation: fp8(clamp(fl32(x * scale)))"""
    return fp8_encode(x.detach().cpu().float() * torch.as_tensor(np.float32(scale)), kind, mode, clamp)


def transpose_bytes(q, qt, off, rows, cols, t_base=None, t_ld=None, swap_tiles=False):
    """qt[t_base + c t_ld + r] = q[off + r cols + c] for the [rows][cols] block at byte offset off (uint8 numpy arrays, in place).
    Defaults: a whole weight (t_base = off, t_ld = rows).  swap_tiles (a mutant): inside every 64 x 64 tile the block is NOT transposed."""
    t_base = off if t_base is None else t_base
    t_ld = rows if t_ld is None else t_ld
    blk = q[off:off + rows * cols].reshape(rows, cols)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    if swap_tiles:
        r, c = (r // 64) * 64 + c % 64, (c // 64) * 64 + r % 64
    qt[t_base + c * t_ld + r] = blk
    return qt


# ------------------------------------------------------------------------------------------- the shadow fixture
SENTINEL_BYTE = 0xA5
PAD = 64                           # sentinel elements between two segments (offsets stay multiples of 64, as the model pads)
# e4m3 ties, subnormals, signed zeros and values beyond 448, as p' * 64 of the planted elements (scale 64 is a power of two: exact)
PLANTED = (1.0625, -1.0625, 1.1875, 17.0, -19.0, 2.0 ** -10, -3 * 2.0 ** -10, 2.0 ** -9, 7 * 2.0 ** -9, -5 * 2.0 ** -9, 0.0, -0.0,
           448.0, -448.0, 456.0, 464.0, 500.0, -1.0e4, 479.9, 2.0 ** -6, 2.0 ** -6 - 2.0 ** -10, 15 * 2.0 ** -10, -2.0 ** -11, 1e-30, -1e-30)


def shadow_fixture(seed=3):
    """A flat layout that walks every path of the update's fp8 shadow, with its inputs and tables (CPU tensors / lists):
      seg 0   W_a  [64][64]    slot 0, scale 64, wd 0, PLANTED values (g = m = v = 0 there: p' = p exactly)     one tile
      seg 1   bias 37          no shadow
      seg 2   W_b  [128][64]   slot 1, scale 8960: |p' scale| passes 448 and saturates                           one tile column
      seg 3   4097 elements    no shadow
      seg 4   W_c  [64][192]   slot 2, scale 37
      seg 5   W_d  [192][128]  slot 3, scale 3000
      seg 6   5 elements       no shadow
      seg 7-9 fused [192][128] as three 64-row bands, slot 4, scale 6000 (saturates), seg_t_ld 192, seg_t_base = offset + band's first row
      seg 10  W_e  [48][80]    slot 5, scale 64, wd 0, seg_in 0: shadowed, no transposed copy; PLANTED values
      seg 11  1 element        no shadow
      slot 6  never updated: its scale and amax words must stay."""
    spec = [("W_a", 64, 64, 0, True), ("bias", 37, 0, -1, False), ("W_b", 128, 64, 1, True), ("vec", 4097, 0, -1, False),
            ("W_c", 64, 192, 2, True), ("W_d", 192, 128, 3, True), ("v5", 5, 0, -1, False),
            ("Q", 64, 128, 4, True), ("K", 64, 128, 4, True), ("V", 64, 128, 4, True), ("W_e", 48, 80, 5, False), ("one", 1, 0, -1, False)]
    scales = [64.0, 8960.0, 37.0, 3000.0, 6000.0, 64.0, 1.0]
    pairs = [(1e-3, 0.0), (1.5e-5, 0.01), (1e-3, 0.01), (1.5e-5, 0.0)]
    off, lens, slot, seg_in, t_base, t_ld, lr, wd, weights, top = [], [], [], [], [], [], [], [], [], 0
    for i, (name, a, b, sl, tr) in enumerate(spec):
        n = a * b if b else a
        fused = name in ("Q", "K", "V")
        if not (fused and name != "Q"):
            top = (top + 63) // 64 * 64 + (PAD if i else 0)
        off.append(top)
        lens.append(n)
        slot.append(sl)
        seg_in.append(b if tr else 0)
        if fused:
            band = "QKV".index(name)
            t_base.append(off[i - band] + 64 * band)
            t_ld.append(192)
            if band == 2:
                weights.append((off[i - 2], 192, 128, True))
        else:
            t_base.append(top if tr else 0)
            t_ld.append(a if tr else 0)
            if sl >= 0:
                weights.append((top, a, b, tr))
        planted = name in ("W_a", "W_e")
        l, w = (1e-3, 0.0) if planted else pairs[i % 4]
        lr.append(l)
        wd.append(w)
        top += n
    total = (top + 63) // 64 * 64 + PAD
    gen = torch.Generator().manual_seed(seed)
    p = 0.02 * torch.randn(total, generator=gen)
    g = torch.randn(total, generator=gen) * 1e-3
    m = torch.randn(total, generator=gen) * 1e-4
    v = torch.rand(total, generator=gen) * 1e-6
    inside = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    planted_idx = []
    for si in (0, 10):
        for k, val in enumerate(PLANTED):
            e = off[si] + (5 + 131 * k) % lens[si]
            p[e] = float(np.float32(val / 64.0))
            g[e] = m[e] = v[e] = 0.0
            planted_idx.append(e)
    return dict(off=off, len=lens, slot=slot, seg_in=seg_in, t_base=t_base, t_ld=t_ld, lr=lr, wd=wd, scales=scales, weights=weights,
                total=total, p=p, g=g, m=m, v=v, inside=inside, planted=planted_idx, n_slots=len(scales))


def per_element(fx, values):
    """a per-segment list -> a per-element fp32 tensor over the flat layout (0 in the padding)"""
    out = torch.zeros(fx["total"])
    for o, n, x in zip(fx["off"], fx["len"], values):
        out[o:o + n] = x
    return out


def shadow_model(fx, p_new, p_old=None, transposed=True, mutate=None):
    """What the update must leave in q, qt (uint8 [total], SENTINEL_BYTE where nothing is written) and max |p'| per slot (fp32 [n_slots],
    0 for a slot no segment has), from the fp32 p' it wrote.  mutate (one of SHADOW_MUTANTS): the wrong kernels the bit comparison
    must catch -- old_p (quantised from the weights before the step), amax_old_p, truncate, unclamped (0x7F / 0xFF appear),
    tile_swapped (not transposed inside the 64 x 64 tile), band_base (a band's seg_t_base without the band's first row)."""
    assert mutate is None or mutate in SHADOW_MUTANTS
    p_new = p_new.detach().cpu().float()
    src = p_old.detach().cpu().float() if mutate == "old_p" else p_new
    q = np.full(fx["total"], SENTINEL_BYTE, dtype=np.uint8)
    qt = np.full(fx["total"], SENTINEL_BYTE, dtype=np.uint8)
    amax = torch.zeros(fx["n_slots"])
    for i, (o, n, sl) in enumerate(zip(fx["off"], fx["len"], fx["slot"])):
        if sl < 0:
            continue
        q[o:o + n] = q8(src[o:o + n], fx["scales"][sl], mode="trunc" if mutate == "truncate" else "rne", clamp=mutate != "unclamped").numpy()
        a_src = p_old.detach().cpu().float() if mutate == "amax_old_p" else p_new
        amax[sl] = max(float(amax[sl]), float(a_src[o:o + n].abs().max()))
        if transposed and fx["seg_in"][i] > 0:
            cols = fx["seg_in"][i]
            base = fx["t_base"][i]
            if mutate == "band_base":
                base = _band_weight_off(fx, i) if fx["t_ld"][i] != n // cols else base
            transpose_bytes(q, qt, o, n // cols, cols, t_base=base, t_ld=fx["t_ld"][i], swap_tiles=mutate == "tile_swapped")
    return torch.from_numpy(q), torch.from_numpy(qt), amax


def _band_weight_off(fx, i):
    """byte offset of the fused weight that band i belongs to"""
    j = i
    while j > 0 and fx["slot"][j - 1] == fx["slot"][i]:
        j -= 1
    return fx["off"][j]
