"""Python handle of the native step engine (crct_engine_* in include/crct_hip.h).

One ``forward`` call = embeddings + 24 encoder steps + heads + loss on the current HIP stream;
``backward`` = the gradients of all 524 used tensors accumulated into the flat fp32 gradient buffer,
optionally segment by segment so the caller can launch gradient all-reduces in between.
"""
import contextlib
import ctypes as C

import torch

from . import lib as L
from .layout import model_variant, parameter_table


def model_dims(cfg, params, cls_dropout=0.1):
    d = L.ModelDims()
    d.vocab, d.n_pos, d.n_types = cfg.vocab_size, cfg.max_position_embeddings, cfg.plotqa_vocab_types
    d.H, d.L, d.heads, d.I = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size
    d.Fv, d.Hv, d.Lv, d.v_heads, d.Iv = (cfg.v_feature_size, cfg.v_hidden_size, cfg.v_num_hidden_layers,
                                         cfg.v_num_attention_heads, cfg.v_intermediate_size)
    d.Hb, d.b_heads, d.n_color = cfg.bi_hidden_size, cfg.bi_num_attention_heads, params["categories"] + 1
    d.n_conn = len(cfg.v_biattention_id)
    for i, (v, t) in enumerate(zip(cfg.v_biattention_id, cfg.t_biattention_id)):
        d.v_biatt[i], d.t_biatt[i] = v, t
    d.fusion_sum = int(cfg.fusion_method == "sum")
    d.with_coattention = int(bool(cfg.with_coattention))
    d.p_hidden, d.p_attn = cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob
    d.p_v_hidden, d.p_v_attn = cfg.v_hidden_dropout_prob, cfg.v_attention_probs_dropout_prob
    d.p_cls = cls_dropout
    return d


class StepEngine(object):
    def __init__(self, cfg, params, max_B, max_T, max_V, device, cls_dropout=0.1):
        self.lib = L.load()
        self.cfg, self.params = cfg, params
        self.table, self.total = parameter_table(cfg, params)
        self.max = (int(max_B), int(max_T), int(max_V))
        names = "\n".join(e.name for e in self.table).encode()
        offs = (C.c_int64 * len(self.table))(*[e.offset for e in self.table])
        # size 0 marks the tensors that never receive a gradient: they are left out of the backward segments' ranges
        sizes = (C.c_int64 * len(self.table))(*[e.numel if e.used else 0 for e in self.table])
        dims = model_dims(cfg, params, cls_dropout)
        kind, reg = model_variant(params)
        self.variant = (kind, reg)
        if (kind, reg) == ("plotqa", "plotqa"):
            self.handle = self.lib.crct_engine_create(C.byref(dims), names, offs, sizes, len(self.table), *self.max)
        else:                      # dvqa / figure_qa: crct_engine_create_variant with the dataset / regressor kind and dvqa_floats
            var = L.Variant()
            var.dataset, var.regressor = L.DATASET_KINDS[kind], L.REGRESSOR_KINDS[reg]
            vals = [float(v) for v in params.get("dvqa_floats", ())]
            if reg == "ce" and len(vals) != L.CE_CLASSES:
                raise ValueError("CE_REG needs params['dvqa_floats'] with %d values (got %d)" % (L.CE_CLASSES, len(vals)))
            if len(vals) > L.CE_CLASSES:
                raise ValueError("params['dvqa_floats'] holds %d values, at most %d are supported" % (len(vals), L.CE_CLASSES))
            if kind == "dvqa" and reg == "plotqa" and not vals:
                raise ValueError("dataset 'dvqa' snaps evaluation outputs to params['dvqa_floats'] (vilbert.py:1619-1625): it is required")
            var.n_values = len(vals)
            for i, v in enumerate(vals):
                var.values[i] = v
            self.handle = self.lib.crct_engine_create_variant(C.byref(dims), names, offs, sizes, len(self.table), *self.max, C.byref(var))
        if not self.handle:
            raise RuntimeError("crct_engine_create failed: %s" % self.lib.crct_last_error().decode())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the CRCT step engine runs on an MI355X only (device=%s); there is no CPU fallback" % device)
        self.ws_bytes = self.lib.crct_engine_workspace_bytes(self.handle)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.n_segments = self.lib.crct_engine_num_segments(self.handle)
        self.segments = []
        lo, hi = C.c_int64(), C.c_int64()
        for s in range(self.n_segments):
            L.check(self.lib.crct_engine_segment_range(self.handle, s, C.byref(lo), C.byref(hi)), "segment_range")
            self.segments.append((lo.value, hi.value))
        B = self.max[0]
        # step outputs in ONE buffer [stats 24 | reg 5*maxB | logits 2*maxB] so that a snapshot is a single copy
        self.NS = 24                                   # 17 used: see CrctHeadArgs.stats (8 step values + the 9 floats of train.py:181)
        self.out = torch.zeros(self.NS + 7 * B, device=self.device)
        self.stats, self.reg = self.out[:self.NS], self.out[self.NS:self.NS + 5 * B].view(5, B)
        self.logits = self.out[self.NS + 5 * B:].view(B, 2)
        self._keep = None
        self._owned_key = None
        self._staged, self._op_handle = None, None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.crct_engine_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # -- batch marshalling: tensors must already be on the device with the dtypes of the C ABI
    def _batch(self, t):
        b = L.Batch()
        b.tokens, b.segments, b.loc = L.ptr(t["tokens"]), L.ptr(t["segments"]), L.ptr(t["loc"])
        b.image_feat, b.image_loc, b.image_target = L.ptr(t["image_feat"]), L.ptr(t["image_loc"]), L.ptr(t["image_target"])
        # key masks: ready-made uint8 masks, or what the data loader ships (the engine builds the masks itself)
        b.text_keymask, b.image_keymask = L.ptr(t.get("text_keymask")), L.ptr(t.get("image_keymask"))
        if t.get("sep_indices") is not None:
            b.sep_indices, b.hist_len, b.sep_stride = L.ptr(t["sep_indices"]), L.ptr(t["hist_len"]), t["sep_indices"].shape[1]
        b.image_mask = L.ptr(t.get("image_mask"))
        b.image_feat_bf16 = int(t["image_feat"].dtype == torch.bfloat16)
        b.R, b.labels = L.ptr(t["R"]), L.ptr(t.get("labels"))
        b.B, b.T, b.V = t["tokens"].shape[0], t["tokens"].shape[1], t["image_feat"].shape[1]
        return b

    def _cfg(self, step):
        c = L.StepCfg()
        c.training, c.use_l1, c.kind_l1 = int(step["training"]), int(step["use_l1"]), int(step["kind_l1"])
        c.tol_margin, c.nsp_coeff, c.reg_coeff = step["tol_margin"], step["nsp_coeff"], step["reg_coeff"]
        c.grad_scale = step.get("grad_scale", 1.0)
        c.wgrad_overwrite = int(bool(step.get("wgrad_overwrite", False)))
        c.grads_bf16 = L.ptr(step.get("grads_bf16")) if c.wgrad_overwrite else None
        c.seed = int(step["seed"])
        c.residual_fp32 = int(bool(step.get("residual_fp32", True)))
        c.g_nsp_dev, c.g_reg_dev, c.g_loss_dev = L.ptr(step.get("g_nsp")), L.ptr(step.get("g_reg")), L.ptr(step.get("g_loss"))
        f8 = step.get("fp8")
        if f8 is not None:          # (flat e4m3 weight shadow, weight scales, activation scales, activation amax): device tensors
            c.fp8 = int(step.get("fp8_mode", 1))
            c.params_fp8, c.fp8_w_scale, c.fp8_act_scale, c.fp8_act_amax = (L.ptr(t) for t in f8)
        f8b = step.get("fp8_bwd")
        if f8b is not None and f8 is not None:      # (mode, transposed e4m3 weight shadow, gradient scales, gradient amax)
            c.fp8_bwd = int(f8b[0])
            c.params_fp8_t, c.fp8_grad_scale, c.fp8_grad_amax = (L.ptr(t) for t in f8b[1:4])
            c.fp8_wgrad = int(bool(f8b[4])) if len(f8b) > 4 else 0
        evs = step.get("seg_events")
        if evs is not None:
            arr = (C.c_void_p * len(evs))(*[ev.cuda_event for ev in evs])
            step["_seg_events_keepalive"] = arr
            c.seg_ready_events = C.cast(arr, C.c_void_p)
        done = step.get("seg_done_events")
        if done is not None:
            arr = (C.c_void_p * len(done))(*[ev.cuda_event for ev in done])
            step["_seg_done_keepalive"] = arr
            c.seg_done_events = C.cast(arr, C.c_void_p)
        mask = step.get("seg_done_mask")
        if mask is not None:
            arr = (C.c_int32 * len(mask))(*[int(bool(m)) for m in mask])
            step["_seg_mask_keepalive"] = arr
            c.seg_done_mask = C.cast(arr, C.c_void_p)
        cb = step.get("seg_enqueued")
        if cb is not None:          # python callable(seg): wrapped once per call; exceptions are kept and re-raised after the engine call
            err = step.setdefault("_seg_enqueued_errors", [])

            def tramp(seg, _user, cb=cb, err=err):
                try:
                    cb(int(seg))
                except BaseException as ex:       # noqa: BLE001 -- must not unwind through the C frame
                    err.append(ex)
            fn = L.SEG_ENQUEUED_FN(tramp)
            step["_seg_enqueued_keepalive"] = fn
            c.seg_enqueued = C.cast(fn, C.c_void_p)
        return c

    # -- per-pass requests: four families of buffers, each standing in the engine until replaced; `requests` pairs set and clear
    def _f32(self, who, name, t, align=0):
        """The pointer of an optional contiguous fp32 device tensor, optionally `align`-byte aligned, as the C ABI takes it."""
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or (align and t.data_ptr() % align)):
            raise ValueError("%s: %s must be a contiguous%s fp32 tensor on the device" % (who, name, ", %d-byte aligned" % align if align else ""))
        return L.ptr(t)

    def _fit_workspace(self, keep):
        """Grow ``workspace`` to the size the library reports now, with its bytes where ``keep``; it never shrinks."""
        self.ws_bytes = self.lib.crct_engine_workspace_bytes(self.handle)
        if self.workspace.numel() < self.ws_bytes:
            grown = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
            if keep:
                grown[:self.workspace.numel()].copy_(self.workspace)
            self.workspace = grown

    def set_ln_addend(self, on):
        """How the block-closing GEMMs of the fp32 residual stream get their fp32 addend (crct_engine_set_ln_addend): True (default)
        = rebuilt in the epilogue from the producing LayerNorm's inputs, False = from an fp32 copy the LayerNorm writes.  The copies'
        buffers are part of the workspace only on the second route: it grows here when needed.  Same bits either way."""
        L.check(self.lib.crct_engine_set_ln_addend(self.handle, int(bool(on))), "set_ln_addend")
        self._fit_workspace(keep=False)

    def set_input_grads(self, image_feat=None, image_loc=None, areas=None, txt_loc=None, text_emb=None):
        """Where the backward passes that follow leave the gradients of the step's float inputs (crct_engine_set_input_grads): contiguous
        fp32 device tensors -- image_feat [B, V, Fv], image_loc [B, V, 4], areas [B, V], txt_loc [B, T, 4], text_emb [B, T, H] (the summed
        text embeddings in front of their LayerNorm) -- each written, not accumulated; None = not wanted, no argument = off.  A feature
        gradient needs B * V * Fv fp32 more workspace: it grows here and KEEPS its bytes, since the request usually arrives between
        the forward and the backward of a batch."""
        named = (("d_image_feat", image_feat), ("d_image_loc", image_loc), ("d_areas", areas), ("d_txt_loc", txt_loc), ("d_text_emb", text_emb))
        req = L.InputGrads(**{name: self._f32("set_input_grads", name, t) for name, t in named})
        L.check(self.lib.crct_engine_set_input_grads(self.handle, C.byref(req)), "engine_set_input_grads")
        self._input_grads = (image_feat, image_loc, areas, txt_loc, text_emb)      # the engine holds raw pointers
        self._fit_workspace(keep=True)

    def sequence_outputs(self, text=True, visual=True):
        """The final hidden states of the LAST forward of this engine (crct_engine_sequence_outputs): (sequence_output_t fp32 [B, T, H],
        sequence_output_v fp32 [B, V, Hv]), fresh tensors that own their memory; None where not asked for.  One launch each, rebuilt from
        what the closing LayerNorm left in the workspace; ``.bfloat16()`` of either is the engine's own bf16 state (taps seq_t / seq_v)."""
        if self._keep is None:
            raise RuntimeError("sequence_outputs: run a forward pass on this engine first")
        tensors, _ = self._keep
        B, T = tensors["tokens"].shape
        V = tensors["image_feat"].shape[1]
        seq_t = torch.empty(B, T, self.cfg.hidden_size, dtype=torch.float32, device=self.device) if text else None
        seq_v = torch.empty(B, V, self.cfg.v_hidden_size, dtype=torch.float32, device=self.device) if visual else None
        L.check(self.lib.crct_engine_sequence_outputs(self.handle, self._keep_p32.data_ptr(), self.workspace.data_ptr(), B, T, V,
                                                      L.ptr(seq_t), L.ptr(seq_v), L.current_stream()), "engine_sequence_outputs")
        return seq_t, seq_v

    def set_output_grads(self, seq_t=None, seq_v=None):
        """Upstream gradients of the final hidden states for the backward passes that follow (crct_engine_set_output_grads): contiguous
        fp32 device tensors [B, T, H] / [B, V, Hv], 16-byte aligned; segment 0 adds grad_scale times each onto that stream's running
        hidden gradient.  None = none, no argument = off.  The backward plan does not depend on it."""
        req = L.OutputGrads(d_seq_t=self._f32("set_output_grads", "d_seq_t", seq_t, 16), d_seq_v=self._f32("set_output_grads", "d_seq_v", seq_v, 16))
        L.check(self.lib.crct_engine_set_output_grads(self.handle, C.byref(req)), "engine_set_output_grads")
        self._output_grads = (seq_t, seq_v)      # the engine holds raw pointers

    def set_score_grads(self, logits=None, value=None):
        """Upstream gradients of the answer logits [B, 2] and of the regressed value ``reg[0]`` [B] for the backward passes that follow
        (crct_engine_set_score_grads): contiguous fp32 device tensors; the loss kernel of segment 0 adds grad_scale times each onto its
        per-row seeds, inside its one launch.  None = none, no argument = off.  ``value`` needs the PlotQA regressor: any other variant
        refuses it.  The backward plan does not depend on it."""
        req = L.ScoreGrads(d_logits=self._f32("set_score_grads", "d_logits", logits), d_value=self._f32("set_score_grads", "d_value", value))
        L.check(self.lib.crct_engine_set_score_grads(self.handle, C.byref(req)), "engine_set_score_grads")
        self._score_grads = (logits, value)      # the engine holds raw pointers

    def set_attention_map_grads(self, requests=()):
        """Upstream gradients of attention maps for the backward passes that follow (crct_engine_set_attention_map_grads): a list of
        ``(kind, index, direction, tensor)`` -- kind / index / direction as ``attention_probs``, the tensor a contiguous fp32 device tensor
        of that map's shape.  Each layer's backward adds grad_scale times the map's contribution onto its own dq / dk, two launches per
        map behind its attention backward.  No argument = off.  The statistics scratch grows the workspace here and KEEPS its bytes
        (the request usually arrives between the forward and the backward of a batch).  The backward plan does not depend on it."""
        reqs = [self.map_key(r[:3]) + (r[3],) for r in requests]
        arr = (L.AttnMapGrad * max(len(reqs), 1))()
        for r, (kind, index, direction, t) in zip(arr, reqs):
            r.kind, r.index, r.direction, r.d_probs = kind, index, direction, self._f32("set_attention_map_grads", (kind, index, direction), t)
        L.check(self.lib.crct_engine_set_attention_map_grads(self.handle, arr if reqs else None, len(reqs)), "engine_set_attention_map_grads")
        self._map_grads = [t for _, _, _, t in reqs]      # the engine holds raw pointers
        self._fit_workspace(keep=True)

    @contextlib.contextmanager
    def requests(self, input_grads=None, output_grads=None, score_grads=None, attention_map_grads=None):
        """The requests of ONE backward pass: sets the families it is given -- a dict of that setter's keyword arguments, for
        ``attention_map_grads`` its list -- and on the way out clears exactly those, in reverse order, also when the body raises.  A family
        left None is not touched: a request standing from before stays.  The plan and the workspace size the library reports follow the
        requests both ways; the workspace tensor keeps what it grew to."""
        given = ((self.set_input_grads, input_grads), (self.set_output_grads, output_grads), (self.set_score_grads, score_grads),
                 (self.set_attention_map_grads, attention_map_grads))
        done = []
        try:
            for setter, arg in given:
                if arg is not None:
                    setter(**arg) if isinstance(arg, dict) else setter(arg)
                    done.append(setter)
            yield self
        finally:
            for setter in reversed(done):
                setter()

    MAP_KINDS = ("text", "visual", "conn")      # an attention's kind by number (AttnSite.kind in csrc/engine.cpp)

    @classmethod
    def map_key(cls, item):
        """``(kind, index[, direction])``, kind by name or number, as three ints (what names no kind passes through: the library refuses it)."""
        kind, index, direction = (tuple(item) + (0,))[:3]
        kind = cls.MAP_KINDS.index(kind) if kind in cls.MAP_KINDS else kind
        return kind if isinstance(kind, str) else int(kind), int(index), int(direction)

    def map_shape(self, kind, direction, B, T, V):
        """Shape of the attention map of a kind (by number) and direction at batch sizes B, T, V; None for what names no kind."""
        cfg = self.cfg
        return {0: (B, cfg.num_attention_heads, T, T), 1: (B, cfg.v_num_attention_heads, V, V),
                2: (B, cfg.bi_num_attention_heads, V, T) if direction else (B, cfg.bi_num_attention_heads, T, V)}.get(kind)

    def set_site_policy(self, site, kind, cfg=-1, split_k=0, phase=-1):
        """Launch policy of one GEMM site (crct_engine_set_site_policy): ``site`` / ``kind`` by name (crct.lib.SITE_NAMES /
        KIND_NAMES) or number, ``phase`` 0 = text-only part of the schedule, 1 = beside the visual stream, -1 = both."""
        s = L.SITE_NAMES.index(site) if isinstance(site, str) else int(site)
        k = L.KIND_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        L.check(self.lib.crct_engine_set_site_policy(self.handle, s, k, int(phase), int(cfg), int(split_k)), "set_site_policy")

    def fp8_layout(self):
        """(number of activation scale sites, [(flat offset, numel)] of the weights with an e4m3 shadow; index = scale slot)."""
        n = self.lib.crct_engine_fp8_weights(self.handle, None, None, 0)
        off, num = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
        if n > 0:
            assert self.lib.crct_engine_fp8_weights(self.handle, off, num, n) == n
        return self.lib.crct_engine_fp8_sites(self.handle), list(zip(off[:n], num[:n]))

    def set_trainable(self, flags):
        """One flag per table entry (crct_engine_set_trainable); None = every tensor has a gradient."""
        key = None if flags is None or all(flags) else tuple(bool(f) for f in flags)
        if key == getattr(self, "_trainable_key", None):
            return
        arr = None if key is None else (C.c_uint8 * len(key))(*[int(f) for f in key])
        L.check(self.lib.crct_engine_set_trainable(self.handle, arr, len(self.table)), "engine_set_trainable")
        self._trainable_key = key

    def backward_plan(self):
        """Per backward segment (runs, text input gradient, visual input gradient, weight-gradient GEMMs left out) under the current
        flags (crct_engine_backward_plan)."""
        out = (C.c_int32 * (4 * self.n_segments))()
        n = self.lib.crct_engine_backward_plan(self.handle, out, self.n_segments)
        assert n == self.n_segments
        return [(bool(out[4 * i]), bool(out[4 * i + 1]), bool(out[4 * i + 2]), int(out[4 * i + 3])) for i in range(n)]

    def grad_segments(self, without_grad=()):
        """``segments`` narrowed to what a pass under the current flags produces: per segment the hull of its tensors with gradient,
        an empty range for a segment that does not run or has none (``without_grad``: names of the tensors without gradient)."""
        if not without_grad:
            return list(self.segments)
        plan = self.backward_plan()
        ents = sorted((e for e in self.table if e.used and e.name not in without_grad), key=lambda e: e.offset)
        out = []
        for (lo, hi), pl in zip(self.segments, plan):
            mine = [e for e in ents if lo <= e.offset < hi] if pl[0] else []
            out.append((mine[0].offset, mine[-1].offset + mine[-1].numel) if mine else (lo, lo))
        return out

    def wgrad_owned(self):
        """(offsets, numels) of the weight gradients the engine overwrites under CrctStepCfg.wgrad_overwrite: fixed by the
        layout at engine creation (every Linear weight produced by exactly one weight-gradient GEMM per pass)."""
        return [list(x) for x in self.wgrad_owned_key()]

    def wgrad_owned_key(self):
        if self._owned_key is None:
            n = self.lib.crct_engine_wgrad_owned(self.handle, None, None, 0)
            off, num = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
            if n > 0:
                assert self.lib.crct_engine_wgrad_owned(self.handle, off, num, n) == n
            self._owned_key = (tuple(off[:n]), tuple(num[:n]))
        return self._owned_key

    # -- the two engine calls go through the registered torch ops (torch.ops.crct.step_forward / step_backward, crct/torch_ops.py);
    #    the step configuration holds scalars, event handles and fp8 state, so it is staged here rather than passed as tensors
    def staged_step(self):
        return self._staged

    def forward(self, p32, p16, tensors, step):
        from . import torch_ops as T
        if self._op_handle is None:
            self._op_handle = T.engine_handle(self)
        self._staged = step
        torch.ops.crct.step_forward(self._op_handle, p32, p16, T.pack_batch(tensors))
        return self.outputs_of(self.out, tensors["tokens"].shape[0])

    def backward(self, p32, p16, g32, tensors, step, seg=-1):
        from . import torch_ops as T
        if self._op_handle is None:
            self._op_handle = T.engine_handle(self)
        self._staged = step
        torch.ops.crct.step_backward(self._op_handle, p32, p16, g32, T.pack_batch(tensors), int(seg))

    def _set_areas(self, tensors):
        if self.variant[0] != "plotqa":
            L.check(self.lib.crct_engine_set_areas(self.handle, L.ptr(tensors.get("areas"))), "engine_set_areas")
        elif tensors.get("areas") is not None:
            raise ValueError("'areas' belongs to the dvqa / figure_qa image embeddings (vilbert.py:1463-1464, 1488-1489)")

    def forward_native(self, p32, p16, tensors, step):
        B = tensors["tokens"].shape[0]
        self._set_areas(tensors)
        b, c = self._batch(tensors), self._cfg(step)
        self._keep, self._keep_p32 = (tensors, step), p32
        L.check(self.lib.crct_engine_forward(self.handle, p32.data_ptr(), p16.data_ptr(), C.byref(b), C.byref(c),
                                             self.workspace.data_ptr(), self.logits.data_ptr(), self.reg.data_ptr(),
                                             self.stats.data_ptr(), L.current_stream()), "engine_forward")
        return self.outputs_of(self.out, B)

    def attention_probs(self, kind, index, direction=0):
        """Attention map of the LAST forward of this engine (crct_engine_attention_probs), a fresh fp32 tensor: kind 0 / "text" layer
        ``index`` -> [B, heads, T, T]; 1 / "visual" -> [B, v_heads, V, V]; 2 / "conn" connection layer ``index``, direction 0 =
        attention_probs1 [B, bi_heads, T, V] (text queries over visual keys), 1 = attention_probs2 [B, bi_heads, V, T].  Computed
        from the layer's bf16 q / k that the forward left in the workspace, with that forward's key masks and dropout stream."""
        if self._keep is None:
            raise RuntimeError("attention_probs: run a forward pass on this engine first")
        tensors, step = self._keep
        kind, index, direction = self.map_key((kind, index, direction))
        shape = self.map_shape(kind, direction, tensors["tokens"].shape[0], tensors["tokens"].shape[1], tensors["image_feat"].shape[1])
        if shape is None:
            raise ValueError("attention_probs: kind must be 0 / 'text', 1 / 'visual' or 2 / 'conn'; got %r" % (kind,))
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        b, c = self._batch(tensors), self._cfg(dict(step, seg_events=None))
        n = self.lib.crct_engine_attention_probs(self.handle, C.byref(b), C.byref(c), self.workspace.data_ptr(), kind, index,
                                                 direction, out.data_ptr(), out.numel(), L.current_stream())
        if n != out.numel():
            raise RuntimeError("attention_probs(%r, %d, %d): %s" % (kind, index, direction, self.lib.crct_last_error().decode()))
        return out

    def outputs_of(self, out, B):
        """(logits [B,2], reg [5,B], stats [24]) views of an output buffer (``self.out`` or a snapshot of it)."""
        o = self.NS + 5 * self.max[0]
        return out[o:o + 2 * B].view(B, 2), out[self.NS:self.NS + 5 * B].view(5, B), out[:self.NS]

    def snapshot(self, B):
        """The step outputs as tensors of their own (ONE copy kernel): the engine rewrites its buffer on the next call."""
        return self.outputs_of(self.out.clone(), B)

    def backward_native(self, p32, p16, g32, tensors, step, seg=-1):
        self._set_areas(tensors)
        b, c = self._batch(tensors), self._cfg(step)
        L.check(self.lib.crct_engine_backward(self.handle, p32.data_ptr(), p16.data_ptr(), C.byref(b), C.byref(c),
                                              self.workspace.data_ptr(), g32.data_ptr(), self.logits.data_ptr(),
                                              self.reg.data_ptr(), self.stats.data_ptr(), int(seg), L.current_stream()),
                "engine_backward")
        errs = step.get("_seg_enqueued_errors")
        if errs:
            raise errs[0]

    def tap(self, name, B, T, V):
        n_max = B * max(T * self.cfg.hidden_size, V * self.cfg.v_hidden_size)
        out = torch.empty(n_max, dtype=torch.bfloat16, device=self.device)
        n = self.lib.crct_engine_tap(self.handle, self.workspace.data_ptr(), name.encode(), B, T, V, out.data_ptr(), n_max,
                                     L.current_stream())
        if n < 0:
            raise RuntimeError("tap(%s): %s" % (name, self.lib.crct_last_error().decode()))
        width = self.cfg.hidden_size if name.endswith(".t") or name == "seq_t" else self.cfg.v_hidden_size
        return out[:n].view(B, -1, width)
