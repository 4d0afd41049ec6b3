"""The attention-map kernel (csrc/attention_probs.hip, ops.attention_probs) per element against fp64 (-m gpu), under the derived budget of
tests/attention_probs_ref.py (the yardstick tests/test_attention_probs_ref_cpu.py proves).

Every case runs the way the step engine calls the kernel: q and k are column slices of fused [*, 3 H + 8] buffers whose other columns hold
data.  The output sits in an fp32 canvas pre-filled with a sentinel bit pattern, with guard elements before and after: every output
element must be written and nothing outside touched.  Shapes with Tk % 4 == 0 run twice -- at a 16-byte aligned output (the float4
stores) and one element further (the dword stores).  The dropout mask is the host Philox copy's (tests/dropout_ref.py): dropped elements
must be exactly 0, kept ones within budget of P / (1 - p).

Largest |got - fp64| / budget measured on the MI355X (each test prints its own; run with -s):
(not measured yet: no MI355X could be reached while this file was written)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops                 # noqa: E402
import attention_ref as AR            # noqa: E402
import attention_probs_ref as PR      # noqa: E402
import dropout_ref as DR              # noqa: E402

DEV = "cuda"
SEED, SITE = 20241017, 13
SENTINEL = 0x7B7B7B7B                 # fp32 bit pattern (1.3e36) no probability takes
GUARD = 67
B, HEADS = 5, 2                       # five batch rows: every mask_row kind of the 'masks' family, whatever the offset
# (Tq, Tk, starred): 130 x 257 has an odd key-tile count and rows that are not 16-byte aligned
SHAPES = [(1, 1, False), (16, 16, False), (17, 33, True), (20, 36, False), (36, 20, False), (44, 124, True), (124, 44, False),
          (113, 113, False), (130, 257, True)]
STARRED = [(Tq, Tk) for Tq, Tk, star in SHAPES if star]


def _run(family, B, heads, Tq, Tk, d, p, idx, offsets=None):
    """One case at every output offset that takes another store path.  Returns the largest budget ratio."""
    what = "%s B=%d heads=%d %dx%dx%d p=%g" % (family, B, heads, Tq, Tk, d, p)
    H = heads * d
    q, k, _, _, km = AR.make_inputs(family, B, heads, Tq, Tk, d, seed=idx, mask_offset=idx)
    g = torch.Generator().manual_seed(idx)
    bufq = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g))        # the neighbours hold data, not zeros: a kernel that strays reads them
    bufk = AR.bf16(torch.randn(B, Tk, 3 * H + 8, generator=g))
    bufq[:, :, :H], bufk[:, :, H:2 * H] = q, k
    q_, k_, km_ = bufq.to(DEV)[:, :, :H], bufk.to(DEV)[:, :, H:2 * H], km.to(DEV)
    keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
    ref, budget = PR.reference(q, k, km, heads, d, keep=keep, p=p)
    n = B * heads * Tq * Tk
    worst = 0.0
    for off in (offsets if offsets is not None else ((0, 1) if Tk % 4 == 0 else (0,))):
        raw = torch.full((4 + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)          # torch allocations are 16-byte aligned and more
        lo = 4 + off if off else 4
        out = raw[lo:lo + n].view(torch.float32).view(B, heads, Tq, Tk)
        assert (out.data_ptr() % 16 == 0) == (off == 0)
        got = ops.attention_probs(q_, k_, km_, heads, d, p_drop=p, site=SITE, seed=SEED, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        host = raw.cpu()
        tag = "%s [output offset %d]" % (what, off)
        assert bool((host[:lo] == SENTINEL).all()) and bool((host[lo + n:] == SENTINEL).all()), "%s: elements outside the output overwritten" % tag
        never = host[lo:lo + n] == SENTINEL
        assert not bool(never.any()), "%s: %d output elements never written, first at flat index %d" % (tag, int(never.sum()), int(never.nonzero()[0]))
        res = host[lo:lo + n].view(torch.float32).view(B, heads, Tq, Tk)
        worst = max(worst, PR.assert_within(res, ref, budget, tag))
        if keep is not None:
            assert bool((res[~torch.as_tensor(keep).reshape(B, heads, Tq, Tk)] == 0.0).all()), "%s: a dropped element is not exactly 0" % tag
    return worst


@pytest.mark.parametrize("d", [32, 48, 64])
def test_masks_family_at_every_shape_against_fp64(d):
    """The masks family (a random 70 %, every key masked, one key attended in the last tile, an aligned run of keys masked in the middle;
    mask_offset steps with the shape so that all four kinds meet every shape), B = 5, heads = 2."""
    worst = 0.0
    for idx, (Tq, Tk, _) in enumerate(SHAPES):
        worst = max(worst, _run("masks", B, HEADS, Tq, Tk, d, 0.0, idx))
    print("attention_probs masks d=%d: %d shapes, largest |got - fp64| / budget %.2f" % (d, len(SHAPES), worst))


@pytest.mark.parametrize("d", [16, 24])
def test_head_sizes_below_32_and_the_zero_filled_contraction_tail(d):
    """d = 16 (one contraction slice) and d = 24 (the second slice half zero-filled) at 17 x 33 and 20 x 36."""
    worst = 0.0
    for idx, (Tq, Tk) in enumerate(((17, 33), (20, 36))):
        worst = max(worst, _run("masks", B, HEADS, Tq, Tk, d, 0.0, 20 + idx))
    print("attention_probs masks d=%d: largest |got - fp64| / budget %.2f" % (d, worst))


@pytest.mark.parametrize("family", ["peaked", "late_max"])
def test_hard_families_at_the_starred_shapes(family):
    """peaked (q, k at standard deviation 2) and late_max (the row maximum arrives with the last attended key: the running sum of sweep 1 is
    rescaled in the last tile pair) at 17 x 33, 44 x 124 and 130 x 257, head sizes 32 / 48 / 64."""
    worst = 0.0
    for idx, (Tq, Tk) in enumerate(STARRED):
        for d in (32, 48, 64):
            worst = max(worst, _run(family, B, HEADS, Tq, Tk, d, 0.0, 40 + 3 * idx + d // 16))
    print("attention_probs %s: largest |got - fp64| / budget %.2f" % (family, worst))


@pytest.mark.parametrize("d", [32, 48, 64])
def test_dropout_carries_the_forward_mask(d):
    """p = 0.1 at the starred shapes: the keep bits are attn_keep8's (tests/dropout_ref.keep_attention, the numbering the forward kernels
    use), dropped elements exactly 0, kept ones within budget of P / (1 - p)."""
    worst = 0.0
    for idx, (Tq, Tk) in enumerate(STARRED):
        worst = max(worst, _run("masks", B, HEADS, Tq, Tk, d, 0.1, 60 + idx))
    print("attention_probs dropout d=%d: largest |got - fp64| / budget %.2f" % (d, worst))


def test_the_length_limit():
    """512 x 512 x 64, B = 1, heads = 1: the largest K image (74 KB of LDS) and the query tiles of one pair spread over workgroups."""
    worst = _run("masks", 1, 1, 512, 512, 64, 0.0, 80, offsets=(0,))
    print("attention_probs 512x512x64: largest |got - fp64| / budget %.2f" % worst)


def test_default_output_and_argument_checks():
    q, k, _, _, km = AR.make_inputs("flat", 2, 3, 20, 36, 32, seed=3)
    q_, k_, km_ = q.to(DEV), k.to(DEV), km.to(DEV)
    out = ops.attention_probs(q_, k_, km_, 3, 32)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 20, 36) and out.is_contiguous()
    ref, budget = PR.reference(q, k, km, 3, 32)
    PR.assert_within(out, ref, budget, "default output")
    with pytest.raises(RuntimeError, match="attention_probs: out"):
        ops.attention_probs(q_, k_, km_, 3, 32, out=torch.empty(2, 3, 36, 20, device=DEV))
    with pytest.raises(RuntimeError, match="attention_probs: out"):
        ops.attention_probs(q_, k_, km_, 3, 32, out=torch.empty(2, 3, 20, 40, device=DEV)[..., :36])
    with pytest.raises(RuntimeError, match="attention_probs: keymask"):
        ops.attention_probs(q_, k_, km_[:, :20], 3, 32)
    with pytest.raises(RuntimeError, match="attention_probs: q"):
        ops.attention_probs(q_, k_, km_, 2, 32)
    with pytest.raises(RuntimeError, match="head size 72"):
        ops.attention_probs(torch.zeros(1, 4, 72, device=DEV, dtype=torch.bfloat16), torch.zeros(1, 4, 72, device=DEV, dtype=torch.bfloat16),
                            torch.ones(1, 4, device=DEV, dtype=torch.uint8), 1, 72)
