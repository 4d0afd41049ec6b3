"""The backward of an attention map (csrc/attention_probs_bwd.hip, ops.attention_probs_bwd) per element against fp64 (-m gpu), under the
derived budget of tests/attn_map_grad_ref.py (the yardstick tests/test_attn_map_grad_ref_cpu.py proves).

Every case runs the way the step engine calls the kernel: q / k and dq / dk are column slices of fused [*, 3 H + 8] buffers whose other
columns hold data; after the run those columns must hold the same bits.  accumulate = 1 adds onto old values of the contributions' size,
accumulate = 0 writes over values of size 100.  The dropout mask is the host Philox copy's (tests/dropout_ref.py).

Largest |got - fp64| / budget measured on the MI355X over the eight shapes (each test prints its own; run with -s): flat 0.53 (accumulate
0) / 0.54 (accumulate 1), masks 0.59, dropout 0.58."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops                 # noqa: E402
import attention_ref as AR            # noqa: E402
import attn_map_grad_ref as MR        # noqa: E402
import dropout_ref as DR              # noqa: E402

DEV = "cuda"
SEED, SITE = 20250311, 21
IDS = ["x".join(str(v) for v in s) for s in MR.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(family, shape, p):
    """Inputs, keep mask and both references (accumulate 0, 1) of one case, computed once."""
    B, heads, Tq, Tk, d = shape
    # mask_offset 1: batch row 0 of the masks family is the fully masked one (mask_row kind 1), at every B
    q, k, km, G, dq0, dk0 = MR.make_case(family, B, heads, Tq, Tk, d, seed=Tq + 2 * Tk, mask_offset=1)
    keep = DR.keep_attention(SEED, SITE, B * heads, Tq, Tk, p) if p > 0 else None
    refs = {acc: MR.reference(q, k, km, G, MR.C_SCALE, heads, d, keep=keep, p=p, dq_old=dq0 if acc else None, dk_old=dk0 if acc else None)
            for acc in (0, 1)}
    return (q, k, km, G, dq0, dk0), refs


def _run(family, shape, p, acc):
    """One launch pair on fused buffers; returns (dq, dk) on the host after checking the neighbouring columns."""
    B, heads, Tq, Tk, d = shape
    H = heads * d
    (q, k, km, G, dq0, dk0), _ = _case(family, shape, p)
    g = torch.Generator().manual_seed(Tq + Tk)
    bufq, bufk = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g)), AR.bf16(torch.randn(B, Tk, 3 * H + 8, generator=g))
    bufq[:, :, :H], bufk[:, :, H:2 * H] = q, k
    bufdq, bufdk = AR.bf16(torch.randn(B, Tq, 3 * H + 8, generator=g) * 100), AR.bf16(torch.randn(B, Tk, 3 * H + 8, generator=g) * 100)
    if acc:
        bufdq[:, :, :H], bufdk[:, :, H:2 * H] = dq0, dk0
    dq_, dk_ = bufdq.to(DEV), bufdk.to(DEV)
    ops.attention_probs_bwd(bufq.to(DEV)[:, :, :H], bufk.to(DEV)[:, :, H:2 * H], km.to(DEV), G.to(DEV), heads, d,
                            outs=(dq_[:, :, :H], dk_[:, :, H:2 * H]), accumulate=bool(acc), scale=MR.C_SCALE, p_drop=p, site=SITE, seed=SEED)
    torch.cuda.synchronize()
    hq, hk = dq_.cpu(), dk_.cpu()
    assert torch.equal(hq[:, :, H:].view(torch.int16), bufdq[:, :, H:].view(torch.int16)), "columns beside dq overwritten"
    assert torch.equal(hk[:, :, :H].view(torch.int16), bufdk[:, :, :H].view(torch.int16)), "columns in front of dk overwritten"
    assert torch.equal(hk[:, :, 2 * H:].view(torch.int16), bufdk[:, :, 2 * H:].view(torch.int16)), "columns behind dk overwritten"
    return hq[:, :, :H].contiguous(), hk[:, :, H:2 * H].contiguous()


def _check(family, shape, p, acc):
    _, refs = _case(family, shape, p)
    (rq, rk), (bq, bk) = refs[acc]
    dq, dk = _run(family, shape, p, acc)
    what = "%s %s p=%g accumulate=%d" % (family, shape, p, acc)
    return max(MR.assert_within(dq, rq, bq, what + " dq"), MR.assert_within(dk, rk, bk, what + " dk")), (dq, dk)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", MR.SHAPES, ids=IDS)
def test_every_element_against_fp64(shape, acc):
    """flat family, no dropout: every element of dq and dk within its budget, written over (accumulate 0) or added (accumulate 1)."""
    worst, _ = _check("flat", shape, 0.0, acc)
    print("attention_probs_bwd flat %s accumulate=%d: largest |got - fp64| / budget %.2f" % (shape, acc, worst))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=IDS)
def test_a_fully_masked_batch_row_and_the_other_mask_kinds(shape):
    """masks family: batch row 0 has every key masked (uniform probabilities over the real keys, none on the padding), the next one a
    single attended key in the last tile."""
    worst, _ = _check("masks", shape, 0.0, 1)
    print("attention_probs_bwd masks %s: largest |got - fp64| / budget %.2f" % (shape, worst))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=IDS)
def test_dropout_with_the_host_philox_mask(shape):
    """p = 0.1: the keep bits are attn_keep8's (tests/dropout_ref.keep_attention): G counts only where the map kept its element."""
    worst, _ = _check("flat", shape, 0.1, 1)
    print("attention_probs_bwd dropout %s: largest |got - fp64| / budget %.2f" % (shape, worst))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=IDS)
def test_two_runs_are_bit_identical(shape):
    a, b = _run("peaked", shape, 0.1, 1), _run("peaked", shape, 0.1, 1)
    for x, y, name in zip(a, b, ("dq", "dk")):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), name


def test_argument_refusals():
    B, heads, Tq, Tk, d = 2, 3, 20, 36, 32
    q, k, km, G, dq0, dk0 = (t.to(DEV) for t in MR.make_case("flat", B, heads, Tq, Tk, d, seed=3))
    ok = dict(outs=(dq0.clone(), dk0.clone()))
    ops.attention_probs_bwd(q, k, km, G, heads, d, **ok)
    with pytest.raises(RuntimeError, match="attention_probs_bwd: d_probs"):
        ops.attention_probs_bwd(q, k, km, G.transpose(2, 3), heads, d, **ok)
    with pytest.raises(RuntimeError, match="attention_probs_bwd: d_probs"):
        ops.attention_probs_bwd(q, k, km, G[..., :32], heads, d, **ok)
    with pytest.raises(RuntimeError, match="attention_probs_bwd: outs"):
        ops.attention_probs_bwd(q, k, km, G, heads, d, outs=(dk0.clone(), dq0.clone()))
    with pytest.raises(RuntimeError, match="attention_probs_bwd: keymask"):
        ops.attention_probs_bwd(q, k, km[:, :20], G, heads, d, **ok)
    with pytest.raises(RuntimeError, match="attention_probs_bwd: q"):
        ops.attention_probs_bwd(q, k, km, G, 2, d, **ok)
    with pytest.raises(RuntimeError, match="must be finite"):
        ops.attention_probs_bwd(q, k, km, G, heads, d, scale=float("nan"), **ok)
    z = torch.zeros(1, 4, 72, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="head size 72"):
        ops.attention_probs_bwd(z, z, torch.ones(1, 4, device=DEV, dtype=torch.uint8), torch.zeros(1, 1, 4, 4, device=DEV), 1, 72,
                                outs=(z.clone(), z.clone()))
