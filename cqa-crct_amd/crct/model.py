"""Host-side mirror of the reference model surface for the CRCT hot path.

  ``VisualDialogEncoder(params)``           <- CRCT/backbone/encoder_decorator.py:9-54
  ``CrctModel`` (``.bert_pretrained``)      <- BertForMultiModalPreTraining, CRCT/backbone/vilbert.py:1499-1661

Same constructor arguments, same ``forward`` keyword arguments / return tuples, same
``state_dict`` keys, shapes and order (561 entries, incl. the tied ``cls.predictions.decoder.weight``),
same ``named_parameters()`` order (560), so the reference's optimizer construction, checkpoints
(``train.py:284-291``) and step adapter keep working.  Underneath there is no torch compute: all
parameters are views into ONE flat fp32 HBM buffer (+ a bf16 shadow, + a flat fp32 gradient buffer)
and ``forward`` / ``backward`` are single calls into the native step engine (hand-written gfx950
kernels, ``include/crct_hip.h``).  The module refuses to run without the HIP library or off-GPU.
"""
import collections
import ctypes as C
import math
import os

import torch
from torch import nn

from . import lib as L
from . import ops
from .config import BertConfig
from .engine import StepEngine
from .fp8 import AMAX_WINDOW, Fp8State
from .heads import HeadPort, LmPrediction, PredictionHead, _HeadLossFn, _LmScoresFn, lm_rows, region_rows      # noqa: F401 (LmPrediction: importable from here)
from .layout import frozen_tensors, img_loss_coeff, is_frozen, lm_loss_coeff, model_variant, optional_grad, parameter_table


class _Node(nn.Module):
    """Name-only container used to reproduce the reference's dotted parameter names."""

    def forward(self, *a, **k):   # pragma: no cover
        raise RuntimeError("structural node of the CRCT parameter tree; call the model instead")


# Where each family of extra outputs sits behind the six fixed ones of a _StepFn result: three slices of result[6:]
_StepLayout = collections.namedtuple("_StepLayout", "seq scores maps")

# What one step hands out behind the six, as ``CrctModel.forward`` decided it: the sequence outputs (asked for, or read by a prediction head's
# loss or scores), the scores as tensors of their own (``differentiable_scores``), the keys of the requested attention maps
_StepWants = collections.namedtuple("_StepWants", "seq scores map_keys")


class _StepFn(torch.autograd.Function):
    """Autograd bridge.  Differentiable outputs: the COMBINED loss (0-dim, = nsp_coeff * nsp + reg_coeff * mean_B reg_loss,
    computed by the head kernel, encoder_decorator.py:144-153), nsp_loss [1] and the per-row regression loss [B]; backward
    hands their upstream gradients (device tensors, no sync) to the engine, which accumulates every parameter gradient
    into the flat buffer (``param.grad`` are views of it).  The usual case -- only ``loss`` is differentiated -- costs no
    torch kernel besides autograd's own seed: the head kernel scales its built-in seeds by the upstream scalar.

    Everything else that can carry a gradient goes through ONE mechanism, the engine's per-pass requests (``StepEngine.requests``):
    backward collects the buffers autograd asks for and the engine holds them for the duration of the pass; a pass that asks for nothing
    is the plain one, launch for launch.  Inputs: the device tensors of ``image_feat``, ``image_loc``, ``loc`` (the text boxes) and
    ``areas``, the same objects ``tensors`` holds; those that need a gradient get a buffer the pass writes, returned with the dtype and
    shape of the input (``CrctModel._run_backward_with_inputs``) -- it carries whatever the upstream gradient carries (a GradScaler's loss
    scale) and is local: a data-parallel pass never exchanges it.  Extra outputs behind the six, in three families whose places
    ``ctx.layout`` records and ``split`` reads back: the encoder's final hidden states (``model.return_sequence_outputs``), the logits and
    the PlotQA regressor's value (``model.differentiable_scores``) and the requested attention maps (``model.attention_map_outputs``) --
    see those attributes; which of them a call hands out is its ``wants`` argument.  An output without an upstream gradient asks for nothing."""

    @staticmethod
    def forward(ctx, anchor, model, tensors, step, wants, image_feat=None, image_loc=None, loc=None, areas=None):
        # (fp8 data gradients only: the forward pass is the plain bf16 one -- no fp8 state, no copies -- the backward pass gets it)
        fwd_step = {k: v for k, v in step.items() if k != "fp8"} if step.get("fp8_backward_only") else step
        eng = model._engine
        eng.forward(model._flat_p, model._flat_b16, tensors, fwd_step)
        ctx.model, ctx.tensors, ctx.step = model, tensors, step
        ctx.set_materialize_grads(False)
        logits, reg_all, stats = eng.snapshot(tensors["tokens"].shape[0])    # one copy; the engine reuses its buffer
        ctx.mark_non_differentiable(logits, reg_all, stats)
        # the differentiable scalar is a tensor of its own (4 bytes): the reference loop modifies it in place
        # (train.py:204-205 ``loss /= params['batch_multiply']``), which autograd forbids on a view output of a multi-output node
        out = [stats[0].clone(), stats[1:2], reg_all[1], logits, reg_all, stats]     # the rest: views of the snapshot, no copies

        def family(ts):
            out.extend(ts)
            return slice(len(out) - 6 - len(ts), len(out) - 6)
        # the encoder's final hidden states, fresh fp32 tensors (StepEngine.sequence_outputs)
        # (also what the prediction heads read: heads._HeadLossFn / _LmScoresFn hang on them, so their gradients come back as these outputs' upstream)
        seq = family(eng.sequence_outputs() if wants.seq else ())
        # the logits, and the PlotQA regressor's value: tensors of their own (two B-sized copies)
        with_value = model.variant[1] == "plotqa"
        scores = family([t.clone() for t in ((logits, reg_all[0]) if with_value else (logits,))] if wants.scores else ())
        # the requested attention maps, fresh fp32 tensors, one launch each (StepEngine.attention_probs)
        ctx.map_keys = wants.map_keys
        maps = family([eng.attention_probs(*key) for key in ctx.map_keys])
        ctx.layout = model._step_layout = _StepLayout(seq, scores, maps)
        return tuple(out)

    @staticmethod
    def split(model, result):
        """A result of ``apply`` as (the six fixed outputs, sequence outputs, scores, maps)."""
        return (result[:6],) + tuple(result[6:][sl] for sl in model._step_layout)

    @staticmethod
    def backward(ctx, g_loss, g_nsp, g_reg, _gl, _gr, _gs, *g_more):
        model = ctx.model
        step = dict(ctx.step)
        B = ctx.tensors["tokens"].shape[0]
        g_seq, g_scores, g_maps = ([_upstream_f32(g) for g in g_more[sl]] for sl in ctx.layout)
        # what the pass asks of the engine besides the loss: the families with an upstream gradient, as StepEngine.requests takes them
        requests = {}
        if any(g is not None for g in g_seq):
            requests["output_grads"] = dict(zip(("seq_t", "seq_v"), g_seq))
        if any(g is not None for g in g_scores):
            requests["score_grads"] = dict(zip(("logits", "value"), g_scores))      # (autograd hands them over as [B, 2] and [B])
        if any(g is not None for g in g_maps):
            requests["attention_map_grads"] = [key + (g,) for key, g in zip(ctx.map_keys, g_maps) if g is not None]
        if g_nsp is None and g_reg is None:
            if g_loss is None:
                if not requests:
                    return (None,) * 9
                g_loss = torch.zeros(1, device=model._flat_p.device)   # only the sequence outputs / scores / maps are differentiated: the heads get zero loss seeds
            step["g_loss"] = g_loss.reshape(1).float()                 # views / no-ops for the fp32 scalar autograd hands over
        else:                                                          # a caller combining nsp_loss / reg_loss itself
            dev = model._flat_p.device
            gl = g_loss.reshape(1).float() if g_loss is not None else torch.zeros(1, device=dev)
            gn = g_nsp.reshape(1).float() if g_nsp is not None else torch.zeros(1, device=dev)
            gr = g_reg.reshape(B).float() if g_reg is not None else torch.zeros(B, device=dev)
            step["g_nsp"] = (gn + gl * step["nsp_coeff"]).contiguous()
            step["g_reg"] = (gr + gl * (step["reg_coeff"] / B)).contiguous()
        return (None,) * 5 + model._run_backward_with_inputs(ctx.tensors, step, ctx.needs_input_grad[5:9], requests)


def _upstream_f32(g):
    """An upstream gradient as the engine reads it: fp32, contiguous, 16-byte aligned (a no-op for what autograd usually hands over)."""
    if g is None:
        return None
    g = g.float().contiguous()
    return g.clone() if g.data_ptr() % 16 else g


class SequenceMask(object):
    """What the step adapter knows about the text key mask -- ``arange(T) < sep_indices[hist_len] + 1``
    (encoder_decorator.py:118-120) -- handed to the model as ``attention_mask`` instead of the materialised tensor: the
    engine builds the uint8 key mask itself (one launch).  ``materialize()`` gives the reference's tensor."""

    def __init__(self, sep_indices, hist_len, max_len):
        self.sep_indices, self.hist_len, self.max_len = sep_indices, hist_len, int(max_len)

    def materialize(self):
        lengths = torch.gather(self.sep_indices, 1, self.hist_len.view(-1, 1)).squeeze(1) + 1
        rng = torch.arange(0, self.max_len, device=lengths.device).long()
        return rng.unsqueeze(0) < lengths.unsqueeze(1)


class CrctModel(nn.Module):
    def __init__(self, config, params=None):
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError("Parameter config in `CrctModel(config)` should be an instance of class `BertConfig`.")
        # dataset / regressor variant (vilbert.py:1463-1466, 1518-1537): PlotQA, DVQA (PlotQA regressor, CE_REG or none) and FigureQA
        self.variant = model_variant(params)
        if self.variant != ("plotqa", "plotqa") and params.get("fp8", False):
            raise NotImplementedError("params['fp8'] is built for the PlotQA model only; the %s / %s variant trains in bf16" % self.variant)
        self.config, self.params = config, params
        device = torch.device(params.get("device", "cuda"))
        if device.type != "cuda":
            raise RuntimeError("CrctModel needs an MI355X (params['device']=%s): the CRCT step has no CPU path" % device)
        self.table, self.total = parameter_table(config, params)
        # areas_emp (dvqa / figure_qa): its .grad exists only once a pass with `areas` has run since the last clear, as in torch
        self._optional = [e for e in self.table if e.used and optional_grad(e.name)]
        self._optional_live = False
        # tensors WITHOUT gradient in a training pass: frozen by config.fixed_t_layer / fixed_v_layer (vilbert.py:857-881) or by
        # requires_grad_(False).  Their .grad is None, their range of the flat gradient buffer is unspecified and nobody reads it
        # (_sync_trainable, before every training forward; the engine then runs less of its backward)
        self._nograd = frozenset()
        self._nograd_version = 0
        self._trainable_key = None
        self._flags = None
        self._flat_p = torch.zeros(self.total, device=device)
        self._flat_g = torch.zeros(self.total, device=device)
        self._flat_b16 = torch.zeros(self.total, device=device, dtype=torch.bfloat16)
        self._shadow_ver = -1
        self._rebound = None
        self._const_zeros = None
        # fp8 forward (BASELINE configs[4], params['fp8']): e4m3 shadow of the QKV / FFN weights + per-tensor delayed scaling
        self.fp8 = bool(params.get("fp8", False)) if params else False
        # ... and the data-gradient GEMMs of the FFN / attention-output Linears from e5m2 gradients and a transposed e4m3 weight
        # shadow (params['fp8_backward'] = False keeps the round-2 behaviour: fp8 forward, bf16 backward)
        self.fp8_backward = self.fp8 and bool(params.get("fp8_backward", True))
        # ... and the FFN weight gradients from the same fp8 copies (params['fp8_wgrad'] = False: bf16 weight gradients)
        self.fp8_wgrad = self.fp8_backward and bool(params.get("fp8_wgrad", True))
        # params['fp8_forward'] = False (round 4): the forward GEMMs stay on the bf16 operands -- the producers still write the e4m3 /
        # scale state the fp8 BACKWARD GEMMs read (the engine's calibration form of the forward, CrctStepCfg.fp8 = 2, kept on).  What
        # costs an fp8 step its gradient fidelity is the e4m3 rounding of the FORWARD (oracle emulation, tools/lab/mx_emulation.py:
        # median gradient cosine 0.90 forward-only, 0.88 with everything; block scaling does not change it), while fp8 data and weight
        # gradients behind an unrounded forward cost ~0.01: this mode keeps most of the speed (backward is 2/3 of the GEMM work).
        self.fp8_forward = bool(params.get("fp8_forward", True)) if params else True
        # params['residual_fp32'] (default on, round 6): the encoder's residual stream is carried in fp32 like the reference's autocast path
        # carries it -- pre-LayerNorm sums and the residual copy of every LayerNorm output; GEMM operands stay bf16 (CrctStepCfg.residual_fp32).
        # False = rounds 1 - 5: both stored as bf16, which is what cost the bf16 path most of its gradient-cosine deficit.
        self.residual_fp32 = bool(params.get("residual_fp32", True)) if params else True
        self._fp8 = None
        self._entries = {e.name: e for e in self.table}
        self._build_tree()
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self._engine = None
        self._seed, self._calls = int(params.get("seed", 0)) * 1000003 + 12345, 0
        self.cls_dropout = 0.1                       # vilbert.py:1045
        self.sync_stats = True                       # reg[3] as python ints (host sync) like the reference
        self._ddp = None
        self._param_events = None                    # set by FusedAdamW in overlap mode
        self._seg_done = None
        self._grads_dirty = True
        self._wgrad_overwrite_next = False       # set by a lazy clear: the next backward pass writes the owned weight gradients
        self._backward_passes = 0
        self._lazy_plan_key, self._lazy_plan = None, None
        self._grad_waits = None
        self.record_segment_events = False           # set by FusedAdamW's early mode
        self._opt_stream = None
        # token saliency: token ids cannot require grad, so True makes the next backward pass leave ``text_embedding_grad`` -- fp32
        # [B, T, H], the gradient with respect to the summed text embeddings in front of their LayerNorm (replaced by every such pass)
        self.keep_text_embedding_grad = False
        self.text_embedding_grad = None
        # True: every forward also returns ``sequence_output_t`` (fp32 [B, T, H], slot 3 of both tuples: vilbert.py:1659, :1661) and leaves
        # it and ``sequence_output_v`` (fp32 [B, V, Hv]) here -- under grad in the training branch as differentiable outputs of the step
        # (an auxiliary loss on the token states trains the encoder through them), otherwise as plain tensors.  Two launches per forward.
        self.return_sequence_outputs = False
        self.sequence_output_t = None
        self.sequence_output_v = None
        # True: in the training branch under grad the answer logits (slot 5 of the training tuple, the step adapter's ``nsp_scores``) and,
        # where the regressor is the PlotQA one, the regressed value (``reg_out[0]``, the adapter's ``regression[0]``) carry a graph, as the
        # reference's do (vilbert.py:1060, :1644, :1659): a loss the caller writes on them -- label smoothing, distillation, a margin
        # between candidate rows -- trains the model, and ``scores[:, 0].sum().backward()`` with ``image_feat.requires_grad_(True)`` is the
        # saliency of the answer.  The CE regressor's value is a table lookup and the binary-answer models have none: no gradient, as
        # in the reference.  The inference tuple (no labels) stays plain: score saliency without real labels is the training branch with
        # every next_sentence_label -1 (the NSP term is then 0), in eval() or train() as the caller likes.  Two B-sized copies per forward;
        # the backward pass launches what it launched.
        self.differentiable_scores = False
        # [("conn", 0, 0), ("text", 11), ...]: (kind, index[, direction]) as ``StepEngine.attention_probs``.  After every forward
        # ``attention_maps`` holds these maps, keyed (kind, index, direction), as fp32 tensors of their own (one launch each); in the
        # training branch under grad they carry a graph, as the reference's all_attention_mask does (vilbert.py:842-946): a loss on a map
        # -- legend supervision on the co-attention, distillation, an entropy penalty -- trains the query / key projections and everything
        # below them.  The backward pass adds two launches per map that has an upstream gradient.  Not with fp8 data gradients
        # (params['fp8_backward']).  The return tuples are unchanged.
        self.attention_map_outputs = ()
        self.attention_maps = {}
        # params['lm_loss_coeff'] > 0: the masked-LM objective (encoder_decorator.py:148-150, vilbert.py:1016-1037).  In the training
        # branch slot 0 of the tuple is then lm_loss = mean over the n tokens with masked_lm_labels >= 0 of logsumexp(logits) - logits[label],
        # fp32 [1, 1], differentiable under grad; the five cls.predictions.* head tensors and the word table (the tied decoder) get
        # gradients.  The labels are taken where the loader leaves them, on the HOST (a device tensor costs one .cpu() per step): the row
        # list is compacted there and uploaded with one pinned copy, every launch is sized by it.  No label (n == 0): the constant zero of
        # the stub and no launch -- torch's CrossEntropyLoss gives NaN there.  The head runs in bf16, also with params['fp8'].
        # Its Linear weight gradient is always accumulated (the lazy clear zeroes it like a bias).
        self.lm_loss_coeff = lm_loss_coeff(params)
        # True: every forward leaves ``prediction_scores_t`` here and returns it in slot 4 of the training tuple and slot 0 of the inference
        # tuple (vilbert.py:1579, :1659, :1661): the LM head's scores of ALL B * T rows, fp32 [B, T, vocab_size] -- a VIEW into the padded
        # [B * T rounded up to 64, vocab_size rounded up to 64] logits, so NOT contiguous (``.contiguous()`` copies; at B 80, T 124 and the
        # BERT vocabulary the buffer is 1.2 GB).  With or without params['lm_loss_coeff'], params['fp8'] (the head runs in bf16) and
        # labels; under grad in the training branch the scores carry a graph (``_LmScoresFn``): a loss on them trains the encoder through
        # sequence_output_t, the word table through the tied decoder and, with lm_loss_coeff > 0, the five head tensors.  With
        # lm_loss_coeff == 0 those five are no part of the step -- no ``.grad``, not in the optimizer -- and get none here either: then only
        # d / d sequence_output_t and the word table's decoder term flow (the word table is a live tensor either way).  With the loss
        # on too the head runs twice, on the masked rows and on all rows; the loss keeps its launches and bits.
        self.return_lm_scores = False
        self.prediction_scores_t = None
        self._opened_pass = -1
        self._shadow_gen = 0
        # params['img_loss_coeff'] > 0: the masked-region objective, the visual twin of the above (ViLBERT's masked-region classification
        # on BertImagePredictionHead, vilbert.py:1065-1077).  In the training branch slot 1 of the tuple is then img_loss = the mean over the
        # n regions with image_label == 1 (the loader has zeroed their features, utils.py:194-217) of the head's loss against the region's
        # class: hard targets (int64 [B, V] class ids) logsumexp(logits) - logits[c]; soft targets (float [B, V, C], t >= 0)
        # sum_j t_j (log t_j - log_softmax(logits)_j), the original's KLDivLoss on detector distributions.  fp32 [1, 1], differentiable under
        # grad; the six cls.imagePredictions.* tensors get gradients.  The targets are ``image_target`` unless ``image_class`` is given:
        # image_target also indexes color_emb in the region's own INPUT embedding (vilbert.py:1479), so a loader that masks a region puts a
        # placeholder there and the truth in image_class.  image_label is taken on the host; no labelled region: the constant zero and no
        # launch.  The head runs in bf16, also with params['fp8'].  One wave holds a row of logits: v_target_size <= 2048.
        self.img_loss_coeff = img_loss_coeff(params)
        if self.img_loss_coeff > 0.0 and config.v_target_size > self.REGION_MAX_CLASSES:
            raise NotImplementedError("params['img_loss_coeff'] with v_target_size = %d: the masked-region loss kernels hold a row of logits in one "
                                      "wave's registers, at most %d classes" % (config.v_target_size, self.REGION_MAX_CLASSES))
        # the two heads: decoder bias, transform Linear weight / bias, LayerNorm weight / bias, decoder weight (text: the tied word table)
        t, v = "cls.predictions.", "cls.imagePredictions."
        self.text_head = PredictionHead(self, t + "bias", t + "transform.dense.weight", t + "transform.dense.bias", t + "transform.LayerNorm.weight",
                                        t + "transform.LayerNorm.bias", "bert.embeddings.word_embeddings.weight", config.hidden_size, config.vocab_size)
        self.region_head = PredictionHead(self, v + "decoder.bias", v + "transform.dense.weight", v + "transform.dense.bias", v + "transform.LayerNorm.weight",
                                          v + "transform.LayerNorm.bias", v + "decoder.weight", config.v_hidden_size, config.v_target_size)
        self.init_weights(int(params.get("seed", 0)))
        self.register_load_state_dict_post_hook(lambda m, k: m._invalidate_shadow())

    # ------------------------------------------------------------------ parameter tree
    def _build_tree(self):
        word = None
        for e in self.table:
            view = self._flat_p[e.offset:e.offset + e.numel].view(e.shape)
            p = nn.Parameter(view, requires_grad=True)
            node = self
            parts = e.name.split(".")
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, _Node())
                node = node._modules[part]
            node.register_parameter(parts[-1], p)
            if e.used and not optional_grad(e.name):
                p.grad = self._flat_g[e.offset:e.offset + e.numel].view(e.shape)
            if e.name == "bert.embeddings.word_embeddings.weight":
                word = p
        # tied LM decoder weight (vilbert.py:1029): second state_dict key, same Parameter
        node = self._modules["cls"]._modules["predictions"]
        node.add_module("decoder", _Node())
        node._modules["decoder"].register_parameter("weight", word)

    def _params_by_name(self):
        return dict(self.named_parameters())

    @torch.no_grad()
    def init_weights(self, seed=0):
        """init_bert_weights (vilbert.py:1099-1110): N(0, initializer_range) for Linear / Embedding weights,
        zero biases, LayerNorm = (1, 0); the regressor keeps nn.Linear's default init (it is created
        after ``self.apply(self.init_bert_weights)``, vilbert.py:1510-1523)."""
        g = torch.Generator(device=self._flat_p.device).manual_seed(seed)
        for e in self.table:
            v = self._flat_p[e.offset:e.offset + e.numel]
            if e.name.startswith("regressor."):
                fan_in = e.shape[1] if len(e.shape) == 2 else self._entries[e.name[:-4] + "weight"].shape[1]
                bound = 1.0 / math.sqrt(fan_in)
                v.uniform_(-bound, bound, generator=g)
            elif "LayerNorm" in e.name:
                v.fill_(1.0 if e.name.endswith("weight") else 0.0)
            elif e.name.endswith("bias"):
                v.zero_()
            else:
                v.normal_(0.0, self.config.initializer_range, generator=g)
        self._invalidate_shadow()

    def _invalidate_shadow(self):
        self._shadow_ver = -1

    def _param_version(self):
        v = self._flat_p._version
        if self._rebound is not None:                # see _rebind: in-place updates through re-pointed Parameters
            v = (v, sum(p._version for p in self._rebound))
        return v

    def _refresh_shadow(self):
        v = self._param_version()
        if self._shadow_ver != v:
            ops.cast_bf16(self._flat_p, out=self._flat_b16)
            self._shadow_ver = v
            self._shadow_gen += 1
            if self._fp8 is not None:
                self._fp8.requantize(self._flat_p, L.current_stream())

    # ------------------------------------------------------------------ fp8 state (crct/fp8.py)
    FP8_AMAX_WINDOW = AMAX_WINDOW

    def _fp8_state(self, eng):
        """The model's Fp8State, created with the first engine and quantised from the current fp32 weights."""
        if self._fp8 is None:
            self._fp8 = Fp8State(self.table, self.total, self._flat_p.device, eng, self.fp8_backward, self.fp8_wgrad, self.fp8_forward)
            self._fp8.requantize(self._flat_p, L.current_stream())
        return self._fp8

    def _apply(self, fn, recurse=True):
        probe = fn(torch.zeros(1, device=self._flat_p.device))
        if probe.dtype != torch.float32:
            raise RuntimeError("CrctModel keeps fp32 master weights (bf16 compute is internal); .half()/.bfloat16() is not supported")
        if probe.device != self._flat_p.device:
            if probe.device.type != "cuda":
                raise RuntimeError("CrctModel cannot leave the GPU: the CRCT step has no CPU path")
            self._flat_p, self._flat_g, self._flat_b16 = fn(self._flat_p), fn(self._flat_g), self._flat_b16.to(probe.device)
            self._anchor = torch.zeros(1, device=probe.device, requires_grad=True)
            self._engine = None
            # everything bound to the old device goes with the engine: fp8 shadow / scales / chunk tables, segment events, the
            # lazy-clear plan, constants (the fused optimizer drops its own device state when it sees the new buffers)
            self._fp8 = None
            self._seg_done = None
            self._lazy_plan_key, self._lazy_plan = None, None
            self._const_zeros = None
            self._param_events = None
            self._opt_stream = None
            self.text_head.reset()
            self.region_head.reset()
            self._rebind()
        return self

    def _rebind(self):
        """After a move to another device.  The Parameters keep their identity (optimizers may already hold them), so their
        ``.data`` is re-pointed at views of the new flat buffer; such views carry their OWN version counters, so from here
        on the bf16 shadow refresh also watches the parameters' counters (``_refresh_shadow``)."""
        byname = self._params_by_name()
        for e in self.table:
            p = byname[e.name]
            p.data = self._flat_p[e.offset:e.offset + e.numel].view(e.shape)
            if e.used and e.name not in self._nograd and (self._optional_live or not optional_grad(e.name)):
                p.grad = self._flat_g[e.offset:e.offset + e.numel].view(e.shape)
        self._rebound = list(byname.values())
        self._invalidate_shadow()

    # ------------------------------------------------------------------ flat views for the optimizer / DDP
    @property
    def flat_params(self):
        return self._flat_p

    @property
    def flat_grads(self):
        return self._flat_g

    @property
    def flat_shadow(self):
        return self._flat_b16

    def note_params_updated_natively(self):
        """Called by the fused optimizer, which rewrites the flat buffers and the shadow itself."""
        self._shadow_ver = self._param_version()
        self._shadow_gen += 1        # (native writes move no torch version counter: what follows the shadow -- the LM head's padded table -- counts these)

    def zero_flat_grads(self, lazy=False):
        """Clear the gradients.  ``lazy``: only the gradients that backward ACCUMULATES into (biases, LayerNorm, embeddings,
        heads: one launch over ~0.1 GB) -- the Linear weight gradients, which the engine produces with exactly one GEMM
        each, are left as they are and WRITTEN by the next backward pass (CrctStepCfg.wgrad_overwrite).  Their ``.grad``
        therefore holds stale values between ``zero_grad()`` and ``backward()``; the values after backward are bit-identical
        to the eager path.  Falls back to the full fill until one backward pass has run."""
        self._set_optional_grads(False)
        self._opened_pass = -1
        plan = self._lazy_zero_plan() if lazy else None
        if plan is None:
            self._flat_g.zero_()
            self._full_clears = getattr(self, "_full_clears", 0) + 1       # crct/ddp.py: NaN-filled views of owned gradients are gone
            self._wgrad_overwrite_next = False
            return
        off, num, blk_seg, blk_off, n_blk = plan
        L.check(L.load().crct_zero_runs(self._flat_g.data_ptr(), off.data_ptr(), num.data_ptr(), blk_seg.data_ptr(),
                                        blk_off.data_ptr(), n_blk, L.current_stream()), "zero_runs")
        self._wgrad_overwrite_next = True

    def _set_optional_grads(self, live):
        """Attach (live) or drop the ``.grad`` views of the areas_emp tensors (their flat gradient stays zero while dropped)."""
        self._optional_live = bool(live)
        if not self._optional:
            return
        if getattr(self, "_optional_params", None) is None:      # the Parameters keep their identity (see _rebind): looked up once
            byname = self._params_by_name()
            self._optional_params = [byname[e.name] for e in self._optional]
        for e, p in zip(self._optional, self._optional_params):
            p.grad = self._flat_g[e.offset:e.offset + e.numel].view(e.shape) if live and e.name not in self._nograd else None

    @property
    def optional_grads_live(self):
        """False: no pass since the last clear carried ``areas`` -- areas_emp has no gradient and an optimizer leaves it alone."""
        return self._optional_live

    @property
    def optional_entries(self):
        return self._optional

    def non_owned_grad_runs(self):
        """Host list of (offset, numel) runs of the flat gradient buffer that backward ACCUMULATES into (everything but the Linear
        weight gradients the engine owns); None before the first engine exists.  Same runs as the lazy clear's."""
        if self._lazy_zero_plan() is None:
            return None
        return list(self._lazy_runs)

    def _lazy_zero_plan(self):
        """Device tables for crct_zero_runs over the complement of the engine's owned weight gradients.  The owned set is
        fixed by the layout (crct_engine_wgrad_owned), so one plan serves every engine this model creates; it is keyed on
        the set itself and ``_run_backward`` re-checks the key against the engine that actually runs the pass."""
        eng = self._engine
        if eng is None:
            return None
        key = eng.wgrad_owned_key()
        if self._lazy_plan_key == key:
            return self._lazy_plan
        owned = list(zip(*key)) if key[0] else []
        starts = [o for o, _ in owned]
        import bisect
        runs = []
        for e in sorted((e for e in self.table if e.used), key=lambda e: e.offset):
            k = bisect.bisect_right(starts, e.offset) - 1
            if k >= 0 and e.offset + e.numel <= owned[k][0] + owned[k][1]:      # a fused QKV weight is one owned range over three tensors
                continue
            if runs and runs[-1][0] + runs[-1][1] == e.offset:
                runs[-1][1] += e.numel
            else:
                runs.append([e.offset, e.numel])
        self._lazy_runs = [tuple(r) for r in runs]
        plan = None
        if owned and runs:
            dev = self._flat_g.device
            num_host = torch.tensor([r[1] for r in runs], dtype=torch.int64)
            lib = L.load()
            n_blk = lib.crct_adamw_plan(num_host.data_ptr(), len(runs), None, None, 0)
            blk_seg = torch.empty(n_blk, dtype=torch.int32)
            blk_off = torch.empty(n_blk, dtype=torch.int64)
            lib.crct_adamw_plan(num_host.data_ptr(), len(runs), blk_seg.data_ptr(), blk_off.data_ptr(), n_blk)
            plan = (torch.tensor([r[0] for r in runs], dtype=torch.int64, device=dev), num_host.to(dev), blk_seg.to(dev),
                    blk_off.to(dev), int(n_blk))
        self._lazy_plan_key, self._lazy_plan = key, plan
        return plan

    # ------------------------------------------------------------------ tensors without gradient
    @property
    def tensors_without_grad(self):
        """Names of the gradient-receiving tensors that the last training forward found frozen (config or ``requires_grad``)."""
        return self._nograd

    def _sync_trainable(self, eng):
        """Before a training forward: which tensors have a gradient in this pass.  Cached on (fixed_t_layer, fixed_v_layer, every
        ``requires_grad``), so an unchanged model costs one tuple comparison; on a change the ``.grad`` views are set / cleared (a
        tensor that gets its gradient back gets a zeroed view of the flat buffer) and the engine is told."""
        if getattr(self, "_used_params", None) is None:
            byname = self._params_by_name()
            self._used_params = [(e, byname[e.name]) for e in self.table if e.used]
            self._used_only = [p for _, p in self._used_params]
        cfg = self.config
        key = (int(cfg.fixed_t_layer), int(cfg.fixed_v_layer), tuple([p.requires_grad for p in self._used_only]))
        if key != self._trainable_key:
            pre = frozen_tensors(cfg)
            new = frozenset(e.name for e, p in self._used_params if not p.requires_grad or is_frozen(pre, e.name))
            if self.fp8 and new:
                # the fused optimizer keeps the e4m3 shadow and its scales current for every shadowed weight it updates: not built
                _, shadowed = eng.fp8_layout()
                for e, _ in self._used_params:
                    if e.name in new and any(o <= e.offset < o + n for o, n in shadowed):
                        raise NotImplementedError("params['fp8'] with '%s' without gradient (fixed_t_layer / fixed_v_layer / requires_grad_(False)): "
                                                  "freezing a weight that has an e4m3 shadow is not supported; train in bf16" % e.name)
            old = self._nograd
            self._nograd = new
            for e, p in self._used_params:
                if e.name in new:
                    p.grad = None
                elif e.name in old and (self._optional_live or not optional_grad(e.name)):
                    self._flat_g[e.offset:e.offset + e.numel].zero_()          # its range held anything while it had no gradient
                    p.grad = self._flat_g[e.offset:e.offset + e.numel].view(e.shape)
            self._flags = [e.name not in new for e in self.table] if new else None
            self._trainable_key = key
            self._nograd_version += 1
        eng.set_trainable(self._flags)

    def _ensure_grad_views(self):
        """``optimizer.zero_grad()`` of stock torch sets ``.grad = None``: re-attach the views and clear.  A tensor without gradient
        (``_sync_trainable``) has ``.grad = None`` on purpose and is not a sign of that."""
        missing = False
        byname = None
        for e in self.table:
            if not e.used or optional_grad(e.name) or e.name in self._nograd:
                continue
            if byname is None:
                byname = self._params_by_name()
            if byname[e.name].grad is None:
                missing = True
                break
        if missing:
            self._flat_g.zero_()
            self._wgrad_overwrite_next = False
            for e in self.table:
                if e.used and not optional_grad(e.name) and e.name not in self._nograd:
                    byname[e.name].grad = self._flat_g[e.offset:e.offset + e.numel].view(e.shape)
            self._set_optional_grads(False)

    # ------------------------------------------------------------------ engine plumbing
    def _get_engine(self, B, T, V):
        eng = self._engine
        if eng is None or B > eng.max[0] or T > eng.max[1] or V > eng.max[2]:
            mb = max(B, eng.max[0] if eng else 0)
            mt = max(T, eng.max[1] if eng else 0)
            mv = max(V, eng.max[2] if eng else 0)
            self._engine = StepEngine(self.config, self.params, mb, mt, mv, self._flat_p.device, self.cls_dropout)
            for pol in getattr(self, "site_policy", ()):          # developer / test overrides of the per-site launch policy
                self._engine.set_site_policy(**pol)
            if getattr(self, "wgrad_workgroups", None) is not None:      # (target, max rows) of crct_engine_set_wgrad_workgroups
                L.check(self._engine.lib.crct_engine_set_wgrad_workgroups(self._engine.handle, int(self.wgrad_workgroups[0]), int(self.wgrad_workgroups[1])), "set_wgrad_workgroups")
            if getattr(self, "wgrad_flush", None) is not None:    # where a layer's weight gradients leave for the side stream (crct_engine_set_wgrad_flush)
                L.check(self._engine.lib.crct_engine_set_wgrad_flush(self._engine.handle, int(self.wgrad_flush)), "set_wgrad_flush")
            if getattr(self, "ln_addend", None) is not None:      # fp32 residual addend rebuilt by the GEMM (True) or written by the LayerNorm (crct_engine_set_ln_addend)
                self._engine.set_ln_addend(self.ln_addend)
            mode = getattr(self, "stream_mode", None)             # (use_visual_stream, use_wgrad_streams) of crct_engine_set_streams
            if mode is not None:
                L.check(self._engine.lib.crct_engine_set_streams(self._engine.handle, int(mode[0]), int(mode[1])), "set_streams")
        return self._engine

    def aux_stream(self):
        """THE side stream of the host-side glue: the optimizer's overlapped update runs on it during the next forward, the
        data-parallel exchange (pack, collectives) during backward -- one stream, because MI355X schedules HIP streams onto
        4 hardware queues and streams that share a queue are serialised: the engine's internal streams already use them."""
        if getattr(self, "_aux_stream", None) is None or self._aux_stream.device != self._flat_p.device or self._aux_engine is not self._engine:
            if self._engine is None:
                raise RuntimeError("the auxiliary stream belongs to the step engine: run a forward pass first")
            n = C.c_int(0)
            ptr = self._engine.lib.crct_engine_aux_stream(self._engine.handle, L.current_stream(), C.byref(n))
            if not ptr:
                raise RuntimeError("crct_engine_aux_stream failed: %s" % self._engine.lib.crct_last_error().decode())
            self._aux_stream = torch.cuda.ExternalStream(ptr, device=self._flat_p.device)
            self._aux_engine, self.queue_classes = self._engine, int(n.value)
        return self._aux_stream

    def segment_done_events(self):
        """4 events per backward segment, recorded by the engine on its internal streams when the segment is enqueued."""
        if self._seg_done is None:
            from .events import DeviceEvent
            self._seg_done = [DeviceEvent() for _ in range(4 * self._engine.n_segments)]
        return self._seg_done

    def take_segment_done_events(self):
        """For the optimizer's early mode: per segment, the callables ``w(stream)`` that order ``stream`` after the
        segment's final gradients of the LAST backward pass (None if that pass did not record them)."""
        waits, self._grad_waits = self._grad_waits, None
        return waits

    def _open_grad_pass(self):
        """What has to happen before anything accumulates into the gradient buffer: the engine's pass does it first thing, a prediction
        head's node -- which autograd runs BEFORE the engine's pass of the same batch -- through ``_open_grad_pass_once``."""
        self._wait_optimizer()
        self._ensure_grad_views()
        self._grads_dirty = True                     # gradients are being accumulated again (optimizer bookkeeping)
        # first pass since a lazy clear: the owned weight gradients hold stale values, which this engine's pass will overwrite if it
        # writes exactly those (an engine rebuilt for a larger batch in between owns the same set: it follows from the layout)
        if self._wgrad_overwrite_next and not (self._lazy_plan_key is not None and self._engine.wgrad_owned_key() == self._lazy_plan_key):
            self._flat_g.zero_()                     # an engine with another owned set: nothing else has been accumulated yet
            self._wgrad_overwrite_next = False

    def _open_grad_pass_once(self):
        """``_open_grad_pass`` once per engine pass, whichever head node runs first: the token is the count of engine passes, which moves
        with ``_run_backward``; a clear in between drops it."""
        if self._opened_pass != self._backward_passes:
            self._opened_pass = self._backward_passes
            self._open_grad_pass()

    def _run_backward(self, tensors, step):
        self._open_grad_pass()
        eng = self._engine
        self._grad_waits = None
        if self._wgrad_overwrite_next:               # a lazy clear is still pending: this pass writes the owned weight gradients,
            step = dict(step, wgrad_overwrite=True)
            self._wgrad_overwrite_next = False       # a further pass before the next clear accumulates
        self._backward_passes = getattr(self, "_backward_passes", 0) + 1
        if tensors.get("areas") is not None and not self._optional_live:
            self._set_optional_grads(True)
        if self._fp8 is not None:
            step = self._fp8.begin_backward(step, L.current_stream())      # fp8 data gradients: step['fp8_bwd']
        if self._ddp is None and self.record_segment_events:
            evs = self.segment_done_events()
            step = dict(step, seg_done_events=evs)
            eng.backward(self._flat_p, self._flat_b16, self._flat_g, tensors, step, -1)
            self._grad_waits = [[(lambda st, ev=ev: ev.wait(st)) for ev in evs[4 * i:4 * i + 4]] for i in range(eng.n_segments)]
            return
        if self._ddp is None:
            if getattr(self, "force_segmented", False):    # developer switch: the DDP call pattern without the collectives
                for i in range(eng.n_segments):
                    eng.backward(self._flat_p, self._flat_b16, self._flat_g, tensors, step, i)
                return
            eng.backward(self._flat_p, self._flat_b16, self._flat_g, tensors, step, -1)
        else:
            self._ddp.backward(self, eng, tensors, step)

    def _run_backward_with_inputs(self, tensors, step, need, requests=None):
        """``_run_backward`` under ONE ``StepEngine.requests``: what ``_StepFn.backward`` collected (``requests``, its keyword arguments) and
        the gradients of the float inputs -- ``need`` = which of (image_feat, image_loc, loc, areas) autograd wants.  Returns those four
        (None where not wanted, and for the features of the dvqa / figure_qa variants, which never read them -- the reference computes
        that term and drops it), each with the dtype and shape of its tensor in ``tensors``; with ``keep_text_embedding_grad`` the pass
        also leaves ``text_embedding_grad``.  A pass that asks for nothing makes no request call into the library at all."""
        want_feat, want_iloc, want_tloc, want_areas = (bool(n) for n in need)
        want_feat = want_feat and self.variant[0] == "plotqa"
        want_areas = want_areas and tensors.get("areas") is not None
        keep_emb = bool(self.keep_text_embedding_grad)
        dev = self._flat_p.device
        B, T = tensors["tokens"].shape

        def buf(like, on):
            return torch.empty(like.shape, dtype=torch.float32, device=dev) if on else None
        d_feat, d_iloc = buf(tensors["image_feat"], want_feat), buf(tensors["image_loc"], want_iloc)
        d_tloc, d_areas = buf(tensors["loc"], want_tloc), buf(tensors.get("areas"), want_areas)
        d_emb = torch.empty(B, T, self.config.hidden_size, dtype=torch.float32, device=dev) if keep_emb else None
        if want_feat or want_iloc or want_tloc or want_areas or keep_emb:
            requests = dict(requests or {}, input_grads=dict(image_feat=d_feat, image_loc=d_iloc, areas=d_areas, txt_loc=d_tloc, text_emb=d_emb))
        with self._engine.requests(**(requests or {})):
            self._run_backward(tensors, step)
        if keep_emb:
            self.text_embedding_grad = d_emb
        if d_feat is not None and tensors["image_feat"].dtype != torch.float32:
            d_feat = d_feat.to(tensors["image_feat"].dtype)
        return d_feat, d_iloc, d_tloc, d_areas

    # ------------------------------------------------------------------ prediction heads (crct/heads.py; see lm_loss_coeff / img_loss_coeff above)
    REGION_MAX_CLASSES = 2048                    # csrc/region_head.hip: 8 float4 chunks per lane of one wave

    def _wait_optimizer(self):
        """Order the current stream after the overlapped optimizer update / gradient memset of the previous step, if there is one."""
        if self._opt_stream is not None:
            from .events import order_streams
            order_streams(self._opt_stream, torch.cuda.current_stream())

    def _head_port(self):
        """All a prediction head sees of the model (``heads.HeadPort``)."""
        world = float(self._ddp.world) if self._ddp is not None and getattr(self._ddp, "world", 1) > 1 else 1.0
        return HeadPort(self._flat_p, self._flat_g, self._flat_b16, self._entries, self._nograd, self._shadow_gen, world,
                        self._wait_optimizer, self._open_grad_pass_once)

    @torch.no_grad()
    def lm_predict(self, labels=None, rows=None, k=5):
        """The LM head's top-k predictions for rows of the LAST forward (any branch; no flag needed: it reads the engine's final text states,
        ``eng.sequence_outputs()``, and the weights as that forward saw them).  Exactly one of ``labels``: [B, T] int64 with -1 = skip, on the host
        or the device (``batch['mask']``; a device tensor costs one ``.cpu()``), compacted as the loss compacts them -- and ``rows``: flat row
        indices into [B * T], without labels.  k in {1, 5, 8}.  Returns an ``LmPrediction``; no row selected: empty tensors and no launch.
        The head runs on the selected rows only (gather, two GEMMs, LayerNorm, one top-k launch per call)."""
        return self.text_head.predict(self._engine, labels, rows, k)

    def _device_inputs(self, input_ids, txt_loc, image_feat, image_loc, token_type_ids, attention_mask,
                       image_attention_mask, image_target, R, labels, areas=None):
        dev = self._flat_p.device

        def to(t, dtype):          # no kernel when the tensor is already on the device with this dtype (resident batches)
            return t.to(device=dev, dtype=dtype, non_blocking=True).contiguous()
        B, T = input_ids.shape
        V = image_feat.shape[1]
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        t = dict(tokens=to(input_ids, torch.int64), segments=to(token_type_ids, torch.int64), loc=to(txt_loc, torch.float32),
                 image_feat=to(image_feat, torch.bfloat16 if image_feat.dtype == torch.bfloat16 else torch.float32),   # bf16 features are taken as shipped
                 image_loc=to(image_loc, torch.float32),
                 image_target=to(image_target, torch.int64), R=to(R, torch.float32))
        # key masks: the engine builds them from sep_indices / hist_len (SequenceMask) and the integer image mask; any other
        # mask tensor is reduced to uint8 here
        if isinstance(attention_mask, SequenceMask):
            t["sep_indices"] = to(attention_mask.sep_indices, torch.int64)
            t["hist_len"] = to(attention_mask.hist_len.reshape(-1), torch.int64)
        elif attention_mask is None:
            t["text_keymask"] = torch.ones(B, T, dtype=torch.uint8, device=dev)
        else:
            t["text_keymask"] = to(attention_mask != 0, torch.uint8)
        if image_attention_mask is None:
            t["image_keymask"] = torch.ones(B, V, dtype=torch.uint8, device=dev)
        elif image_attention_mask.dtype == torch.int64:
            t["image_mask"] = to(image_attention_mask, torch.int64)
        else:
            t["image_keymask"] = to(image_attention_mask != 0, torch.uint8)
        if labels is not None:
            t["labels"] = to(labels.reshape(-1), torch.int64)
        if areas is not None:                      # [B, V, 1] (encoder_decorator.py:93-96) -> fp32 [B][V]
            t["areas"] = to(areas.reshape(B, V), torch.float32)
        return t

    # ------------------------------------------------------------------ forward (vilbert.py:1540-1661)
    def forward(self, input_ids, txt_loc, image_feat, image_loc, sep_indices=None, sep_len=None, token_type_ids=None,
                attention_mask=None, image_attention_mask=None, masked_lm_labels=None, image_label=None, image_target=None,
                next_sentence_label=None, output_all_attention_masks=False, gt_reg=None, areas=None, legend_pred=None, image_class=None):
        if areas is not None and self.variant[0] == "plotqa":
            raise ValueError("'areas' belongs to the figure_qa / dvqa image embeddings (vilbert.py:1463-1464, 1488-1489)")
        if gt_reg is None:
            raise ValueError("gt_reg=[R, kind] is required (vilbert.py:1586)")
        if self.training and float(self.params.get("mask_prob_img", 0.0) or 0.0) > 0.0:
            # vilbert.py:1491-1493 zeroes whole visual elements in training when mask_prob_img > 0; this step has no such masking, and
            # training on without it would train a different model than the one asked for
            raise RuntimeError("params['mask_prob_img'] = %g: masking of visual elements in training (vilbert.py:1491-1493) is not "
                               "supported; set it to 0" % float(self.params["mask_prob_img"]))
        if image_target is None:
            raise ValueError("image_target is required by the image embeddings (vilbert.py:1479)")
        map_keys = self._attention_map_keys()
        if map_keys and self.fp8 and self.fp8_backward:
            raise NotImplementedError("attention_map_outputs with params['fp8_backward']: the e5m2 copies of the fused dq | dk | dv gradients are "
                                      "written by the attention backward itself, so a map's contribution would miss them; set "
                                      "params['fp8_backward'] = False or leave attention_map_outputs empty")
        R, kind = gt_reg[0], gt_reg[1]
        train_branch = masked_lm_labels is not None and next_sentence_label is not None and image_target is not None
        # the masked-LM loss of this batch (host work only; a bad label is refused here, before any launch); None: off, or no token has a label
        text_head, region_head = self.text_head, self.region_head
        lm_job = lm_rows(masked_lm_labels, self.config.vocab_size) if train_branch and self.lm_loss_coeff > 0.0 else None
        lm_job = text_head.upload(lm_job) if lm_job is not None else None
        # ... and the masked-region loss: the targets are image_target unless image_class is given (it takes their place for the loss ONLY)
        region_job = None
        if train_branch and self.img_loss_coeff > 0.0:
            region_job = region_rows(image_label, image_target if image_class is None else image_class,
                                     "image_target" if image_class is None else "image_class", *image_feat.shape[:2], self.config.v_target_size)
            region_job = region_head.upload(region_job) if region_job is not None else None
        # what the step hands out: the sequence outputs on request or for a head's loss or scores, the scores' own tensors, the maps
        want_seq = bool(self.return_sequence_outputs or lm_job is not None or region_job is not None or self.return_lm_scores)
        tensors = self._device_inputs(input_ids, txt_loc, image_feat, image_loc, token_type_ids, attention_mask,
                                      image_attention_mask, image_target, R, next_sentence_label if train_branch else None, areas)
        B, T = tensors["tokens"].shape
        V = tensors["image_feat"].shape[1]
        eng = self._get_engine(B, T, V)
        if train_branch and torch.is_grad_enabled():
            self._sync_trainable(eng)          # which tensors have a gradient in this pass (before any launch: it may refuse)
        self._refresh_shadow()
        self._calls += 1
        p = self.params
        step = dict(training=self.training, use_l1=bool(p["L1"]), kind_l1=(kind == "L1"), tol_margin=float(p["tol_margin"]),
                    nsp_coeff=float(p.get("nsp_loss_coeff", 1.0)), reg_coeff=float(p.get("reg_loss_coeff", 1.0)),
                    seed=(self._seed + self._calls * 7919 + int(p.get("rank", 0)) * 104729) & 0x3FFFFFFFFFFFFFFF,
                    seg_events=self._param_events, residual_fp32=self.residual_fp32)
        self._param_events = None
        dev = self._flat_p.device
        if self.fp8:                                   # step['fp8'] / ['fp8_mode'] / ['fp8_backward_only'], dry pass, activation scales
            self._fp8_state(eng).begin_forward(step, train_branch and torch.is_grad_enabled(), self.training,
                                               lambda dry: eng.forward(self._flat_p, self._flat_b16, tensors, dry))
        attention_maps = None
        if train_branch and torch.is_grad_enabled():
            # the float inputs as autograd inputs; the engine's dict keeps detached aliases of the ones that are part of a graph
            live = (tensors["image_feat"], tensors["image_loc"], tensors["loc"], tensors.get("areas"))
            if any(t is not None and t.requires_grad for t in live):
                tensors = dict(tensors, image_feat=live[0].detach(), image_loc=live[1].detach(), loc=live[2].detach())
                if live[3] is not None:
                    tensors["areas"] = live[3].detach()
            wants = _StepWants(want_seq, bool(self.differentiable_scores), map_keys)
            (loss, nsp, reg_loss, logits, reg, stats), seq, scores, maps = _StepFn.split(self, _StepFn.apply(self._anchor, self, tensors, step, wants, *live))
            lm_loss = _HeadLossFn.apply(seq[0], text_head, lm_job) if lm_job is not None else None
            lm_scores = _LmScoresFn.apply(seq[0], text_head) if self.return_lm_scores else None
            img_loss = _HeadLossFn.apply(seq[1], region_head, region_job) if region_job is not None else None
            value = scores[1] if len(scores) > 1 else None
            if scores:
                logits = scores[0]                     # differentiable_scores: the copies that are part of the graph
        else:
            value = None
            eng.forward(self._flat_p, self._flat_b16, tensors, step)
            logits, reg, stats = eng.snapshot(B)
            loss, nsp, reg_loss = stats[0], stats[1:2], reg[1]
            seq = eng.sequence_outputs() if want_seq else ()
            lm_loss = text_head.loss(seq[0], lm_job)[0] if lm_job is not None else None      # torch.no_grad() in the training branch: forward only
            lm_scores = text_head.scores(seq[0])[0] if self.return_lm_scores else None
            img_loss = region_head.loss(seq[1], region_job)[0] if region_job is not None else None
            maps = [eng.attention_probs(*key) for key in map_keys]
            if output_all_attention_masks and not train_branch:
                attention_maps = self._attention_maps(eng)
        self.attention_maps = dict(zip(map_keys, maps))
        # the combined training loss as the head kernel computed it (differentiable); the step adapter returns it instead
        # of re-deriving it from nsp_loss / reg_loss with five more torch kernels and their autograd nodes
        self.last_loss = loss if train_branch else None
        self.loss_coeffs = (step["nsp_coeff"], step["reg_coeff"])
        self.last_stats = stats
        if self.sync_stats:
            right = (int(stats[4].item()), int(stats[5].item()))          # vilbert.py:1647 (.item() host syncs)
        else:
            right = (stats[4], stats[5])
        reg_out = [reg[0] if value is None else value, reg_loss, reg[2], right, reg[4]]
        if self._const_zeros is None or self._const_zeros[0].device != dev:
            # the placeholder losses of vilbert.py:1583,1652-1653 (lm, image, legend): constant tensors made once, not three
            # fill kernels per step
            self._const_zeros = (torch.zeros(1, 1, device=dev), torch.zeros(1, 1, device=dev), torch.zeros(1, device=dev))
        lm_zero, img_zero, legend_loss = self._const_zeros
        # sequence_output_t in slot 3 of both tuples, on request (return_sequence_outputs); both final states stay on the model
        self.sequence_output_t, self.sequence_output_v = seq if seq and self.return_sequence_outputs else (None, None)
        self.prediction_scores_t = lm_scores                 # (return_lm_scores; None otherwise)
        if train_branch:
            return lm_zero if lm_loss is None else lm_loss, img_zero if img_loss is None else img_loss, nsp, self.sequence_output_t, lm_scores, logits, reg_out, legend_loss   # vilbert.py:1659
        return lm_scores, None, logits, self.sequence_output_t, attention_maps, reg_out, legend_loss               # vilbert.py:1661

    def _attention_map_keys(self):
        """``attention_map_outputs`` as the keys of ``attention_maps``: (kind, index, direction), kind by name, direction 0 by default."""
        keys = []
        for item in self.attention_map_outputs or ():
            kind, index, direction = StepEngine.map_key(item)
            if kind not in (0, 1, 2):
                raise ValueError("attention_map_outputs: kind must be 'text', 'visual' or 'conn'; got %r" % (kind,))
            keys.append((StepEngine.MAP_KINDS[kind], index, direction))
        return tuple(keys)

    def _attention_maps(self, eng):
        """``output_all_attention_masks=True`` (vilbert.py:842-946, :1562): (text maps, visual maps, co-attention maps) of the forward
        that just ran -- one fp32 tensor per text layer [B, heads, T, T] and per visual layer [B, v_heads, V, V] in layer order, one
        (attention_probs1 [B, bi_heads, T, V], attention_probs2 [B, bi_heads, V, T]) pair per connection layer (:725).  Every tensor
        owns its memory.  No forward kernel stores probabilities: each map is computed here by one launch of its own
        (csrc/attention_probs.hip) from the layer's fused q / k / v buffer, which the step engine writes as bf16 in EVERY mode -- the
        fp8 modes quantise the inputs and weights of the projection GEMM, its output stays bf16 (engine.cpp self_fwd / conn_fwd:
        ``Act{a.qkv}`` carries no e4m3 copy) -- so the maps exist for the DVQA / FigureQA variants and all fp8 modes alike.  In
        ``train()`` without labels the maps carry the forward's dropout mask (same seed and sites), as the reference's do."""
        cfg = self.config
        maps_t = [eng.attention_probs(0, i) for i in range(cfg.num_hidden_layers)]
        maps_v = [eng.attention_probs(1, i) for i in range(cfg.v_num_hidden_layers)]
        maps_c = [(eng.attention_probs(2, i, 0), eng.attention_probs(2, i, 1)) for i in range(len(cfg.v_biattention_id))] if cfg.with_coattention else []
        return maps_t, maps_v, maps_c


class VisualDialogEncoder(nn.Module):
    """encoder_decorator.py:9-54.  ``params['model_config']`` must exist (same assertion as :14).

    The reference builds its model with ``from_pretrained('bert-base-uncased', ...)`` (encoder_decorator.py:16), i.e. it STARTS FROM
    BERT-base for the tensors that have a counterpart there (text embeddings, the twelve text layers, the LM head) and downloads the
    archive when it is not cached.  Here the archive is a local path: ``pretrained=`` (or ``params['bert_pretrained']``) names a
    directory holding ``pytorch_model.bin``, a ``.bin`` file or a ``.tar.gz`` archive -- or is a state dict -- and is loaded with the
    reference's rules (crct/pretrained.py: gamma / beta rename, ``bert.`` prefix rule, name-and-shape matching, size mismatch =
    RuntimeError).  Without it the model keeps the ``init_bert_weights`` initialisation -- exactly the state of the reference model
    right before its weight loading (vilbert.py:1205) -- and says so once: that is a different starting point from the reference's."""

    _warned_no_pretrained = False

    def __init__(self, params, config=None, pretrained=None):
        super().__init__()
        if config is None:
            config_path = params["model_config"]
            assert os.path.exists(config_path), "model_config file not found"
            config = BertConfig.from_json_file(config_path)
        self.bert_pretrained = CrctModel(config, params=params)
        if pretrained is None:
            pretrained = params.get("bert_pretrained")
        if pretrained is not None:
            from .pretrained import load_pretrained
            self.pretrained_missing, self.pretrained_unexpected = load_pretrained(self.bert_pretrained, pretrained)
        elif not VisualDialogEncoder._warned_no_pretrained and not params.get("quiet_init", False):
            VisualDialogEncoder._warned_no_pretrained = True
            import warnings
            warnings.warn("VisualDialogEncoder: no BERT-base checkpoint given (pretrained=<path> or params['bert_pretrained']); the model starts "
                          "from init_bert_weights, whereas the reference starts its text stream from bert-base-uncased "
                          "(encoder_decorator.py:16).  Loading a CRCT checkpoint afterwards (train.py:91-130) makes this moot.")
        self.bert_pretrained.train()

    def forward(self, input_ids, txt_loc, image_feat, image_loc, sep_indices=None, sep_len=None, token_type_ids=None,
                attention_mask=None, masked_lm_labels=None, next_sentence_label=None, head_mask=None,
                random_round_indices=None, output_nsp_scores=False, output_lm_scores=False, image_attention_mask=None,
                image_label=None, image_target=None, gt_reg=None, areas=None, legend_pred=None, image_class=None):
        masked_lm_loss = masked_img_loss = nsp_loss = prediction_scores_t = None
        kw = dict(sep_indices=sep_indices, sep_len=sep_len, token_type_ids=token_type_ids, attention_mask=attention_mask,
                  masked_lm_labels=masked_lm_labels, next_sentence_label=next_sentence_label,
                  image_attention_mask=image_attention_mask, image_label=image_label, image_target=image_target,
                  gt_reg=gt_reg, areas=areas, legend_pred=legend_pred, image_class=image_class)
        core = self.bert_pretrained
        was = core.return_lm_scores
        if output_lm_scores:                 # the flag for this call: the appended element is the tensor (encoder_decorator.py:52-53)
            core.return_lm_scores = True
        try:
            if next_sentence_label is not None and masked_lm_labels is not None and image_target is not None:
                masked_lm_loss, masked_img_loss, nsp_loss, _, prediction_scores_t, seq_relationship_score, reg_loss, legend_loss = \
                    core(input_ids, txt_loc, image_feat, image_loc, **kw)
            else:
                prediction_scores_t, _, seq_relationship_score, _, _, reg_loss, legend_loss = \
                    core(input_ids, txt_loc, image_feat, image_loc, **kw)
        finally:
            core.return_lm_scores = was
        out = (masked_lm_loss, masked_img_loss, nsp_loss, seq_relationship_score)
        if output_lm_scores:
            out = out + (prediction_scores_t,)
        return out + (reg_loss, legend_loss)
