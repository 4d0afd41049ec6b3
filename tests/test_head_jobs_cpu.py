"""The host side of the two prediction heads' jobs (crct/heads.py ``lm_rows`` / ``region_rows``), on hand-made CPU tensors: what is refused,
with which text, what is compacted and in which order, and that nothing on a row without a label is ever looked at.  B 2, T = V = 5,
C 7, a vocabulary of 13."""
import math
import re

import pytest
import torch

from crct.heads import HeadJob, lm_rows, region_rows

B, T, V, NC, VOCAB = 2, 5, 5, 7, 13


def lm_labels():
    return torch.tensor([[-1, 4, -1, 0, VOCAB - 1], [7, -1, -1, -1, 7]])


def region_labels():
    """image_label as the loader writes it: 1 = masked region, 0 = the <IMG> row, -1 elsewhere."""
    return torch.tensor([[0, 1, -1, 1, -1], [0, -1, -1, -1, 1]])


def class_ids():
    ids = torch.tensor([[3, 0, 2, NC - 1, 1], [5, 6, 6, 6, 4]])
    ids[region_labels() != 1] = 10 ** 6                # garbage on every row without label 1
    return ids


def soft_targets():
    t = torch.rand(B, V, NC, generator=torch.Generator().manual_seed(1))
    t[0, 1, 2] = 0.0                                   # a zero is a valid soft target
    t[region_labels() != 1] = float("nan")             # garbage on every row without label 1 ...
    t[0, 0] = -1.0                                     # ... of both kinds
    return t


# ------------------------------------------------------------------------------------------------ masked-LM labels
def test_lm_rows_compacts_in_nonzero_order():
    lab = lm_labels()
    job = lm_rows(lab, VOCAB)
    flat = lab.reshape(-1)
    want = (flat >= 0).nonzero().flatten()
    assert isinstance(job, HeadJob) and job.targets is None
    assert job.rows.dtype == torch.int64 and torch.equal(job.rows, want) and job.rows.tolist() == [1, 3, 4, 5, 9]
    assert job.labels.dtype == torch.int64 and torch.equal(job.labels, flat[want]) and job.labels.tolist() == [4, 0, VOCAB - 1, 7, 7]
    assert job.R == 5 and job.inv_n == 1.0 / 5
    assert not job.rows.is_cuda and not job.labels.is_cuda
    one = lm_rows(torch.tensor([[-1, -1, 2, -1, -1], [-1] * 5], dtype=torch.int32), VOCAB)       # any integer dtype, R = 1
    assert one.rows.tolist() == [2] and one.labels.tolist() == [2] and one.R == 1 and one.inv_n == 1.0


def test_lm_rows_without_any_label_is_none():
    assert lm_rows(torch.full((B, T), -1), VOCAB) is None


@pytest.mark.parametrize("bad", [VOCAB, VOCAB + 100, -2, -(10 ** 6)])
def test_lm_rows_refuses_a_bad_token_id(bad):
    lab = lm_labels()
    lab[1, 1] = bad
    text = "masked_lm_labels: %d is neither -1 (no label) nor a token id below vocab_size = %d" % (bad, VOCAB)
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        lm_rows(lab, VOCAB)
    lab[0, 0] = -7 if bad < 0 else VOCAB + 5           # the FIRST bad label in row order is the one named
    with pytest.raises(ValueError, match="^" + re.escape("masked_lm_labels: %d is neither" % int(lab[0, 0]))):
        lm_rows(lab, VOCAB)


# ------------------------------------------------------------------------------------------------ masked regions, class ids
def test_region_rows_hard_targets_compact_in_nonzero_order_and_skip_unlabelled_garbage():
    lab, ids = region_labels(), class_ids()
    job = region_rows(lab, ids, "image_class", B, V, NC)
    want = (lab.reshape(-1) == 1).nonzero().flatten()
    assert isinstance(job, HeadJob) and job.targets is None
    assert job.rows.dtype == torch.int64 and torch.equal(job.rows, want) and job.rows.tolist() == [1, 3, 9]
    assert job.labels.dtype == torch.int64 and job.labels.tolist() == [0, NC - 1, 4]
    assert job.R == 3 and job.inv_n == 1.0 / 3
    flat = region_rows(lab.reshape(-1).to(torch.int32), ids.reshape(-1).to(torch.int32), "image_target", B, V, NC)     # element counts are what is checked
    assert torch.equal(flat.rows, job.rows) and torch.equal(flat.labels, job.labels)


def test_region_rows_without_a_labelled_region_is_none_whatever_the_targets_hold():
    lab = region_labels()
    lab[lab == 1] = -1
    assert region_rows(lab, torch.full((B, V), -5), "image_target", B, V, NC) is None
    assert region_rows(lab, torch.full((B, V, NC), float("nan")), "image_class", B, V, NC) is None
    assert region_rows(lab, torch.zeros(3), "image_class", B, V, NC) is None                     # not even their shape is looked at


def test_region_rows_needs_image_label():
    text = "image_label is required by params['img_loss_coeff'] > 0: 1 on the regions the loader masked (utils.py:194-217)"
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        region_rows(None, class_ids(), "image_target", B, V, NC)


def test_region_rows_refuses_wrong_element_counts_and_shapes():
    lab, ids = region_labels(), class_ids()
    with pytest.raises(ValueError, match="^" + re.escape("image_label has 8 elements, the batch has B * V = 2 * 5 regions") + "$"):
        region_rows(lab[:, :4], ids, "image_target", B, V, NC)
    with pytest.raises(ValueError, match="^" + re.escape("image_target: class ids are [B, V] = [2, 5]; got (2, 4)") + "$"):
        region_rows(lab, ids[:, :4], "image_target", B, V, NC)
    for bad in (torch.zeros(B, V, NC + 1), torch.zeros(B * V, NC), torch.zeros(B, V)):
        text = "image_class: soft targets are [B, V, v_target_size] = [2, 5, 7]; got %s" % (tuple(bad.shape),)
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            region_rows(lab, bad, "image_class", B, V, NC)


@pytest.mark.parametrize("bad", [NC, -1, 10 ** 6])
@pytest.mark.parametrize("keyword", ["image_target", "image_class"])
def test_region_rows_refuses_a_class_id_outside_the_classes_on_a_labelled_row(bad, keyword):
    ids = class_ids()
    ids[1, 4] = bad
    text = "%s: %d on a region with image_label == 1 is no class id in [0, v_target_size = %d)" % (keyword, bad, NC)
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        region_rows(region_labels(), ids, keyword, B, V, NC)


# ------------------------------------------------------------------------------------------------ masked regions, soft targets
def test_region_rows_soft_targets_keep_the_tensor_and_skip_unlabelled_garbage():
    lab, t = region_labels(), soft_targets()
    job = region_rows(lab, t, "image_class", B, V, NC)
    assert job.labels is None and job.rows.tolist() == [1, 3, 9] and job.R == 3 and job.inv_n == 1.0 / 3
    assert tuple(job.targets.shape) == (B * V, NC) and job.targets.data_ptr() == t.data_ptr()    # the caller's tensor, flattened: no copy
    assert math.isnan(float(job.targets[2, 0])) and float(job.targets[0, 0]) == -1.0             # the garbage is still there, unread
    half = region_rows(lab, t.double(), "image_class", B, V, NC)                                 # any floating dtype
    assert half.targets.dtype == torch.float64 and half.rows.tolist() == [1, 3, 9]


@pytest.mark.parametrize("bad", [-1e-6, float("nan"), float("inf"), float("-inf")])
def test_region_rows_refuses_a_negative_or_non_finite_soft_target_on_a_labelled_row(bad):
    t = soft_targets()
    t[1, 4, NC - 1] = bad
    text = "image_class: a soft target on a region with image_label == 1 is negative or not finite"
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        region_rows(region_labels(), t, "image_class", B, V, NC)
