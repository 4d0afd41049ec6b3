"""The two prediction heads of the training step: the masked-LM head on ``sequence_output_t`` (``cls.predictions.*``, decoder tied to the
word table; csrc/lm_head.hip) and the masked-region head on ``sequence_output_v`` (``cls.imagePredictions.*``; csrc/region_head.hip).

Host side only.  ``lm_rows`` / ``region_rows`` check one batch's labels and compact its labelled rows (plain tensor code, no device, no
library); ``PredictionHead`` -- one instance per head -- uploads such a job and runs the ONE head routine (``logits`` / ``grads``) for the
loss, the scores and the predictions; ``_HeadLossFn`` / ``_LmScoresFn`` hang them on the step's sequence outputs.  A head reaches its model
through ``CrctModel._head_port()`` alone.
"""
import collections

import torch

from . import ops

# One batch's labelled rows as a head takes them: flat row indices into [B * T] / [B * V], R of them, 1 / n, and ONE of labels (class or token
# ids [R]: the hard form) and targets (the soft form, region head only: [B * V, C], read in place at ``rows``).  An LM job has targets = None.
# As ``lm_rows`` / ``region_rows`` return it the tensors are the host's (int64; targets where the caller had them); ``PredictionHead.upload``
# gives the device form (int32 from one pinned copy; targets fp32).
HeadJob = collections.namedtuple("HeadJob", "rows labels targets R inv_n")

# What ``CrctModel.lm_predict`` returns: the flat row indices into [B * T] (int32), the k most probable token ids of each row (int32 [R, k], most
# probable first, ties to the smaller id) with their log-probabilities (fp32 [R, k]), and -- with labels, else None -- each row's label
# log-probability (fp32 [R]) and rank (int32 [R]: the number of tokens in front of the label; ``rank < k`` = "label in the top k")
LmPrediction = collections.namedtuple("LmPrediction", "rows ids logprobs label_logprob label_rank")

# All a head sees of its model (``CrctModel._head_port()``): the flat fp32 parameters, gradients and bf16 shadow, the layout entries by name,
# the names without gradient, the shadow's generation, the data-parallel world size (a float), and two calls: order the current stream
# after an overlapped optimizer update; open the gradient pass (once per engine pass).
HeadPort = collections.namedtuple("HeadPort", "p g b16 entries nograd shadow_gen world wait_optimizer open_grad_pass")


def lm_rows(masked_lm_labels, vocab_size):
    """Host side of one batch's masked-LM loss, before any launch: the labels are checked (-1 = no label, else a token id) and the rows
    with a label compacted.  A host ``HeadJob``, or None when no token has a label."""
    lab = masked_lm_labels
    if lab.is_cuda:
        lab = lab.cpu()                                   # the loader leaves them on the host (encoder_decorator.py:85); this is a sync
    lab = lab.reshape(-1).to(torch.int64)
    bad = (lab >= vocab_size) | (lab < -1)
    if bool(bad.any()):
        raise ValueError("masked_lm_labels: %d is neither -1 (no label) nor a token id below vocab_size = %d" % (int(lab[bad][0]), vocab_size))
    rows = (lab >= 0).nonzero().flatten()
    R = int(rows.numel())
    return HeadJob(rows, lab[rows], None, R, 1.0 / R) if R else None


def region_rows(image_label, targets, keyword, B, V, n_classes):
    """Host side of one batch's masked-region loss, before any launch: the rows with image_label == 1 are compacted; their targets
    (``keyword`` names the argument they came from) are checked -- a class id must lie in [0, C), a soft target must be finite and
    >= 0; what other rows hold is never looked at.  A host ``HeadJob`` (soft targets: the caller's tensor as [B * V, C]), or None when
    no region is labelled."""
    if image_label is None:
        raise ValueError("image_label is required by params['img_loss_coeff'] > 0: 1 on the regions the loader masked (utils.py:194-217)")
    lab = image_label.cpu() if image_label.is_cuda else image_label      # a device tensor costs one .cpu(), as for the LM labels
    lab = lab.reshape(-1)
    if lab.numel() != B * V:
        raise ValueError("image_label has %d elements, the batch has B * V = %d * %d regions" % (lab.numel(), B, V))
    rows = (lab == 1).nonzero().flatten()
    R = int(rows.numel())
    if R == 0:
        return None
    if not torch.is_floating_point(targets):
        if targets.numel() != B * V:
            raise ValueError("%s: class ids are [B, V] = [%d, %d]; got %s" % (keyword, B, V, tuple(targets.shape)))
        ids = targets.reshape(-1)
        ids = ids[rows.to(ids.device)].cpu().to(torch.int64)
        bad = (ids < 0) | (ids >= n_classes)
        if bool(bad.any()):
            raise ValueError("%s: %d on a region with image_label == 1 is no class id in [0, v_target_size = %d)" % (keyword, int(ids[bad][0]), n_classes))
        return HeadJob(rows, ids, None, R, 1.0 / R)
    if tuple(targets.shape) != (B, V, n_classes):
        raise ValueError("%s: soft targets are [B, V, v_target_size] = [%d, %d, %d]; got %s" % (keyword, B, V, n_classes, tuple(targets.shape)))
    flat = targets.reshape(B * V, n_classes)
    picked = flat.index_select(0, rows.to(flat.device))
    if bool(((picked < 0) | ~torch.isfinite(picked)).any()):
        raise ValueError("%s: a soft target on a region with image_label == 1 is negative or not finite" % keyword)
    return HeadJob(rows, None, flat, R, 1.0 / R)


class PredictionHead(object):
    """One prediction head: the names of the decoder bias, the transform's Linear weight / bias and LayerNorm weight / bias and the decoder's
    weight (the tied word table for the text head), the hidden width ``H`` and the class count ``C``; and the head's own device state --
    the padded decoder operands with the shadow generation they were made at, the pinned staging buffer of the row upload and, for the
    scores, the identity row lists."""

    def __init__(self, model, bias, w, b, gamma, beta, table, H, C):
        self._port = model._head_port
        self.bias, self.w, self.b, self.gamma, self.beta, self.table, self.H, self.C = bias, w, b, gamma, beta, table, H, C
        self._staging = (None, None)
        self._all_rows = {}
        self.reset()

    def reset(self):
        """Drop what is bound to the model's device (the model moved)."""
        self._pad, self._pad_gen = None, -1

    @staticmethod
    def _view(flat, entry):
        return flat[entry.offset:entry.offset + entry.numel].view(entry.shape)

    # ------------------------------------------------------------------ jobs
    def upload(self, job):
        """A host job of ``lm_rows`` / ``region_rows`` on the device: (rows | labels) as int32 through one pinned, asynchronous copy; a soft
        target tensor as fp32 [B * V, C]."""
        dev = self._port().p.device
        if job.labels is None:
            targets = job.targets.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
            return job._replace(rows=self._upload_i32(dev, job.rows), targets=targets)
        buf = self._upload_i32(dev, job.rows, job.labels)
        return job._replace(rows=buf[:job.R], labels=buf[job.R:])

    def _upload_i32(self, dev, *parts):
        """The host integer tensors ``parts`` (R elements each) as ONE int32 device tensor, through the pinned staging buffer."""
        R = int(parts[0].numel())
        n = len(parts) * R
        host, done = self._staging
        if done is not None:
            done.synchronize()                                # the staging buffer is free again (long done in practice)
        if host is None or host.numel() < n:
            host = torch.empty(max(n, 4096), dtype=torch.int32).pin_memory()
        for i, part in enumerate(parts):
            host[i * R:(i + 1) * R] = part
        out = torch.empty(n, dtype=torch.int32, device=dev)
        out.copy_(host[:n], non_blocking=True)
        done = done or torch.cuda.Event()
        done.record()
        self._staging = (host, done)
        return out

    # ------------------------------------------------------------------ the head routine
    def _operands(self, m):
        """(bf16 [Vp, H] copy of the decoder weight's bf16 shadow -- the word table for the text head -- with zero pad rows, fp32 [Vp] padded
        bias), refreshed whenever the shadow was."""
        if self._pad is None or self._pad_gen != m.shadow_gen:
            self._pad = ops.lm_pad_operands(self._view(m.b16, m.entries[self.table]), self._view(m.p, m.entries[self.bias]), *(self._pad or ()))
            self._pad_gen = m.shadow_gen
        return self._pad

    def logits(self, seq, rows, R):
        """The head on rows ``rows`` (int32 [R], device) of its sequence output ``seq`` (fp32 [B, T, H]): z = LayerNorm(gelu(h W^T + b)),
        logits = z E^T + bias on the padded operands.  Returns (logits fp32 [Rp, Vp] -- rows R .. and columns C .. are padding --, what
        ``grads`` needs).  The one forward of both losses, the scores and the predictions."""
        m = self._port()
        m.wait_optimizer()                   # an overlapped optimizer update may still be writing the head's weights and shadow
        H, e = self.H, m.entries
        table, bias = self._operands(m)
        hb = ops.lm_gather_rows(seq.view(-1, H), rows, R)
        Rp, Vp = hb.shape[0], table.shape[0]
        pre = torch.empty(Rp, H, device=hb.device, dtype=torch.bfloat16)
        a = ops.gemm(hb, self._view(m.b16, e[self.w]), Rp, H, H, bias=self._view(m.p, e[self.b]), act="gelu", preact_out=pre)
        z, mean, rstd = ops.layernorm_fwd(a, self._view(m.p, e[self.gamma]), self._view(m.p, e[self.beta]), eps=1e-12)
        logits = ops.gemm(z, table, Rp, Vp, H, bias=bias, out_f32=True)
        return logits, (hb, pre, a, mean, rstd, z, table)

    def grads(self, m, dL, saved, rows, R, shape):
        """dL bf16 [Rp, Vp] (the gradient of the padded logits, pad rows and columns +0, 1 / world folded in) -> accumulates the gradients of
        the head's five tensors and of its decoder weight (for the text head: the decoder term of the word table), each only where the
        tensor is part of the step and has a gradient, and returns d / d (the head's sequence output), fp32 ``shape``, zero outside
        ``rows``.  The one backward of both losses and the scores."""
        hb, pre, a, mean, rstd, z, table = saved
        H, V = self.H, self.C
        Rp, Vp = dL.shape
        g_bias, g_table, g_gamma, g_beta, g_w, g_b = (
            self._view(m.g, m.entries[name]) if m.entries[name].used and name not in m.nograd else None
            for name in (self.bias, self.table, self.gamma, self.beta, self.w, self.b))
        if g_bias is not None:
            ops.lm_add(g_bias, ops.colsum(dL, Rp, Vp), V, True)
        if g_table is not None:
            ops.lm_decoder_wgrad(dL, z, g_table, V, True)
        dz = ops.gemm(dL, table, Rp, H, Vp, tb=True)
        dx = ops.layernorm_bwd(dz, a, mean, rstd, self._view(m.p, m.entries[self.gamma]), dgamma=g_gamma, dbeta=g_beta, accumulate=True)[0]
        dpre = ops.lm_gelu_bwd(dx, pre)
        if g_w is not None:
            ops.gemm(dpre, hb, H, H, Rp, ta=True, tb=True, out=g_w, accumulate=True)
        if g_b is not None:
            ops.colsum(dpre, Rp, H, out=g_b, accumulate=True)
        # (a data-parallel pass folds 1 / world into the gradient seeds (crct/ddp.py); the engine applies it to the upstream of the sequence
        # output itself, so the row gradients handed back are taken out of it again)
        dh = ops.gemm(dpre, self._view(m.b16, m.entries[self.w]), Rp, H, H, tb=True, out_f32=True, alpha=m.world)
        d_seq = torch.zeros(shape, dtype=torch.float32, device=dh.device)
        ops.lm_scatter_rows(dh, rows, d_seq.view(-1, H), R)
        return d_seq

    # ------------------------------------------------------------------ loss
    def loss(self, seq, job):
        """The head's loss fp32 [1, 1] over the labelled rows of ``seq`` and what the backward needs: ``logits``, then the loss over the C real
        columns.  Hard targets of either head: the vocabulary kernels, which measured no slower than the one-wave-per-row ones at C = 1601
        (EXPERIMENTS.md); soft targets: the one-wave-per-row kernels of csrc/region_head.hip."""
        logits, saved = self.logits(seq, job.rows, job.R)
        if job.targets is None:
            _, lse, loss = ops.lm_ce_fwd(logits, job.labels, job.R, self.C, job.inv_n)
        else:
            _, lse, loss = ops.region_ce_fwd(logits, job.R, self.C, job.inv_n, targets=job.targets, rows=job.rows)
        return loss, (saved, logits, lse)

    def loss_backward(self, job, saved, shape, g):
        """Accumulates the head's parameter gradients (``grads``) and returns d loss / d (its sequence output), fp32 ``shape``, zero outside
        the labelled rows.  Runs before the engine's backward pass of the same batch (autograd orders it so) and opens that pass first."""
        saved, logits, lse = saved
        m = self._port()
        m.open_grad_pass()
        g = g.reshape(1).float()
        if job.targets is None:
            dL = ops.lm_ce_bwd(logits, job.labels, lse, g, job.inv_n / m.world, job.R, self.C)
        else:
            dL = ops.region_ce_bwd(logits, lse, g, job.inv_n / m.world, job.R, self.C, targets=job.targets, rows=job.rows)
        return self.grads(m, dL, saved, job.rows, job.R, shape)

    # ------------------------------------------------------------------ scores and predictions (the text head)
    def scores(self, seq):
        """(prediction_scores_t fp32 [B, T, V], a view of the padded logits; the identity row list; what the backward needs).  All B * T rows go
        through the head; the row list is cached per row count and needs no host labels."""
        B, T, _ = seq.shape
        N = B * T
        rows = self._all_rows.get(N)
        if rows is None or rows.device != seq.device:
            rows = self._all_rows[N] = torch.arange(N, dtype=torch.int32, device=seq.device)
        logits, saved = self.logits(seq, rows, N)
        return logits[:N].view(B, T, logits.shape[1])[:, :, :self.C], rows, saved

    def scores_backward(self, rows, saved, shape, g):
        """d (upstream g on the scores) / d sequence_output_t; the head's and the word table's gradients are accumulated (``grads``).  g is
        taken where autograd left it when its rows are 16-byte aligned fp32 with a stride that is a multiple of 4, else through one copy
        into such rows (vocab_size itself need not be a multiple of 4)."""
        m = self._port()
        m.open_grad_pass()
        V, N, table = self.C, int(rows.numel()), saved[-1]
        g = g.reshape(N, V)
        if g.dtype != torch.float32 or g.stride(1) != 1 or g.stride(0) % 4 or g.data_ptr() % 16:
            buf = torch.empty(N, ops.pad64(V), dtype=torch.float32, device=g.device)
            buf[:, :V].copy_(g)
            g = buf[:, :V]
        dL = ops.lm_scores_grad_pack(g, N, ops.pad64(max(N, 1)), V, table.shape[0], 1.0 / m.world)
        return self.grads(m, dL, saved, rows, N, shape)

    @torch.no_grad()
    def predict(self, eng, labels=None, rows=None, k=5):
        """``CrctModel.lm_predict`` on engine ``eng``'s last forward."""
        if (labels is None) == (rows is None):
            raise ValueError("lm_predict: give exactly one of labels= ([B, T], -1 = skip) and rows= (flat row indices)")
        if int(k) not in (1, 5, 8):
            raise ValueError("lm_predict: k = %r must be 1, 5 or 8" % (k,))
        if eng is None or eng._keep is None:
            raise RuntimeError("lm_predict: run a forward pass first")
        B, T = eng._keep[0]["tokens"].shape
        dev = self._port().p.device
        if labels is not None:
            if labels.numel() != B * T:
                raise ValueError("lm_predict: labels has %d elements, the last forward had B * T = %d * %d rows" % (labels.numel(), B, T))
            job = lm_rows(labels, self.C)
            job = self.upload(job) if job is not None else None
            row_idx, lab, R = (job.rows, job.labels, job.R) if job is not None else (None, None, 0)
        else:
            r64 = torch.as_tensor(rows).reshape(-1).to(torch.int64).cpu()
            R, lab = int(r64.numel()), None
            if R and bool(((r64 < 0) | (r64 >= B * T)).any()):
                raise ValueError("lm_predict: rows must lie in [0, B * T = %d)" % (B * T))
            row_idx = r64.to(torch.int32).to(dev) if R else None
        if R == 0:
            e_i, e_f = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, device=dev)
            return LmPrediction(e_i, e_i.reshape(0, int(k)), e_f.reshape(0, int(k)), e_f if labels is not None else None, e_i if labels is not None else None)
        logits, _ = self.logits(eng.sequence_outputs(visual=False)[0], row_idx, R)
        ids, logprob, _, lab_lp, lab_rank = ops.lm_topk_rows(logits, R, self.C, int(k), lab)
        return LmPrediction(row_idx, ids, logprob, lab_lp, lab_rank)


class _HeadLossFn(torch.autograd.Function):
    """A head's loss (params['lm_loss_coeff'] / params['img_loss_coeff'] > 0) as a node of its own on the head's sequence output, a
    differentiable output of the step: forward = ``PredictionHead.loss``, backward = ``PredictionHead.loss_backward``, which accumulates the
    head's parameter gradients into the flat gradient buffer and RETURNS d loss / d sequence output -- autograd hands it to the step's
    backward as the upstream gradient of that output, i.e. through the engine's output-gradient request, so the encoder, the co-attention
    and any requested input gradient see it.  The upstream gradient of the loss (a GradScaler's scale, a caller's weight) is a device
    scalar the gradient kernel reads: no ``.item()``."""

    @staticmethod
    def forward(ctx, seq, head, job):
        loss, ctx.saved = head.loss(seq, job)
        ctx.head, ctx.job, ctx.shape = head, job, seq.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.head.loss_backward(ctx.job, ctx.saved, ctx.shape, g), None, None


class _LmScoresFn(torch.autograd.Function):
    """``prediction_scores_t`` (``CrctModel.return_lm_scores``) as a node on ``sequence_output_t``, beside the loss's: forward =
    ``PredictionHead.scores`` over ALL B * T rows, the output a [B, T, V] view of the padded logits; backward packs the upstream [B, T, V]
    gradient into the bf16 [Rp, Vp] form the loss's gradient kernel leaves (``ops.lm_scores_grad_pack``) and runs the same chain,
    ``PredictionHead.grads``: head gradients and the decoder term where the tensor has a gradient, d / d sequence_output_t returned."""

    @staticmethod
    def forward(ctx, seq_t, head):
        scores, rows, ctx.saved = head.scores(seq_t)
        ctx.head, ctx.rows, ctx.shape = head, rows, seq_t.shape
        ctx.set_materialize_grads(False)
        return scores

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return ctx.head.scores_backward(ctx.rows, ctx.saved, ctx.shape, g), None
