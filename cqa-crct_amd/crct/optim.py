"""Optimizer / LR-schedule surface of the reference (CRCT/utils.py:11-29, 228-249) on flat buffers.

``get_optimizer(params, model)`` returns a ``torch.optim.Optimizer`` with the reference's layout --
ONE param group per tensor in ``named_parameters()`` order, lr = ``params['lr']`` for BERT-base
language tensors else ``params['image_lr']``, weight decay 0 for names containing ``bias`` /
``LayerNorm.bias`` / ``LayerNorm.weight`` -- so ``optimizer.state_dict()`` / ``load_state_dict()``
round-trip with reference checkpoints (train.py:105-130, 284-291).  The update itself is ONE HIP
kernel over the flat parameter / gradient / moment buffers (crct_adamw_step), which also refreshes
the bf16 weight shadow; tensors that never receive a gradient are skipped, as torch.optim.AdamW
skips ``grad is None`` parameters.
"""
import contextlib
import json
import os

import numpy as np
import torch
from torch.optim.lr_scheduler import _LRScheduler

from . import lib as L
from . import ops
from .events import order_streams
from .layout import NO_DECAY, is_language_weight


class WarmupLinearScheduleNonZero(_LRScheduler):
    """Linear warm-up to the base lr over ``warmup_steps``, then linear decay towards 0 at ``t_total``,
    floored at ``min_lr`` (utils.py:11-29)."""

    def __init__(self, optimizer, warmup_steps, t_total, min_lr=1.3e-5, last_epoch=-1):
        self.warmup_steps, self.t_total, self.min_lr = warmup_steps, t_total, min_lr
        super().__init__(optimizer, last_epoch=last_epoch)

    def get_lr(self):
        step = self.last_epoch
        if step < self.warmup_steps:
            f = float(step) / float(max(1, self.warmup_steps))
        else:
            f = max(0, float(self.t_total - step) / float(max(1.0, self.t_total - self.warmup_steps)))
        return [b * f if (b * f) > self.min_lr else self.min_lr for b in self.base_lrs]


def _crct_core(model):
    core = getattr(model, "bert_pretrained", model)
    core = getattr(core, "module", core)
    if not hasattr(core, "flat_params"):
        core = getattr(core, "bert_pretrained", core)
    return core


def active_blocks(blk_seg, blk_off, active):
    """The chunk table (``ops.adamw_plan``: per block its segment and its offset inside it, blocks in segment order) cut down to
    the segments with ``active[segment]``: the blocks of the others are dropped, segment numbers stay -- the per-segment arrays
    (offsets, lengths, lr, weight decay) are indexed as before.  Host tensors in, host tensors out."""
    keep = torch.as_tensor(active, dtype=torch.bool)[blk_seg.long()]
    return blk_seg[keep].contiguous(), blk_off[keep].contiguous()


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics, one launch.  ``param_groups`` keep the caller's layout."""

    def __init__(self, param_groups, model, lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(param_groups, defaults)
        self.core = _crct_core(model)
        core = self.core
        dev = core.flat_params.device
        self._m = torch.zeros_like(core.flat_params)
        self._v = torch.zeros_like(core.flat_params)
        self._step = 0
        byname = dict(core.named_parameters())
        self._used = [e for e in core.table if e.used]
        ids = {id(byname[e.name]): e for e in self._used}
        self._group_of = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if id(p) in ids:
                    self._group_of[ids[id(p)].name] = gi
        self._segs = sorted([e for e in self._used if e.name in self._group_of], key=lambda e: e.offset)
        to_dev = lambda v, dt: torch.as_tensor(v, dtype=dt).to(dev)   # noqa: E731
        self._seg_off = to_dev([e.offset for e in self._segs], torch.int64)
        self._seg_len = to_dev([e.numel for e in self._segs], torch.int64)
        blk_seg, blk_off = ops.adamw_plan([e.numel for e in self._segs])
        self._blk_seg, self._blk_off = blk_seg.to(dev), blk_off.to(dev)
        # tensors without gradient (CrctModel.tensors_without_grad: frozen by the config or by requires_grad_(False)) are skipped as
        # torch.optim.AdamW skips ``grad is None``: the full table is kept on the host and the device table rebuilt without their
        # blocks whenever that set changes (_sync_active) -- weights, moments, step counters and bf16 shadow stay untouched
        self._blk_full = (blk_seg, blk_off)
        self._active_ver = 0
        # areas_emp (dvqa / figure_qa): block range of each of its segments -- a step after passes without `areas` leaves its weights
        # and moments untouched, as torch.optim.AdamW does for a None gradient
        self._index_optional(blk_seg)
        self._lr_host = torch.empty(len(self._segs), dtype=torch.float32).pin_memory()
        self._wd_host = torch.empty(len(self._segs), dtype=torch.float32).pin_memory()
        self._lr_dev = torch.empty(len(self._segs), dtype=torch.float32, device=dev)
        self._wd_dev = torch.empty(len(self._segs), dtype=torch.float32, device=dev)
        self._last = None
        self._step_dev, self._amp_arg, self._amp_keep = None, None, None
        self._g16 = None                     # bf16 gradient source of the running update (data-parallel bf16 exchange), else None
        # clip_grad_norm_: the pending clip coefficient (device scalar, folded into exactly the next step()) and what it came from
        self._clip = None
        self._clip_partials = self._clip_seg_norms = self._clip_keep = None
        # crct/ddp.py: while THIS optimizer is alive and covers every gradient, a bf16 exchange need not write the weight gradients
        # back to fp32 (a weak reference: an optimizer that was built and discarded must not change what .grad holds)
        import weakref
        core._fused_optimizer = weakref.ref(self)
        self._model_ref = weakref.ref(model)         # ema_state_dict() speaks the keys of the model the optimizer was built for
        # overlap mode: the update runs as one launch per engine backward-segment on its own stream, in first-use
        # order, each followed by an event; the next forward waits for segment s right before it needs it, so
        # AdamW (HBM-bound, ~1.2 ms) and the gradient memset overlap the next step's forward
        self.overlap = False
        self.overlap_workgroups = 256        # throttle of the overlapped launches (one workgroup per CU), 0 = full width
        self.full_width_first = 1            # this many of the first overlapped launches (embeddings first) run unthrottled
        self.launch_groups = 0               # > 0: the overlapped update in that many launches instead of one per backward segment
        self.fp8_transpose_workgroups = 256  # same for the transposed fp8 weight shadow that follows the update (fp8 backward)
        # the update zeroes every gradient element it has consumed; the zero_grad() that follows is then free.  Off by
        # default: torch optimizers leave .grad untouched in step() (a caller may still want to read it there)
        self.fuse_zero_grad = False
        # zero_grad() clears only what backward accumulates into; the Linear weight gradients are overwritten by the next
        # backward pass (no 0.96 GB fill, no read-modify-write in the weight-gradient GEMMs: -0.3 ms per step).  Their
        # .grad is stale (not zero) between zero_grad() and backward(); set False for the eager fill.
        self.lazy_zero_grad = True
        # early mode (with overlap): the update of a segment starts as soon as the backward pass has finished that
        # segment's gradients (the engine marks it with events), i.e. it overlaps the REST OF BACKWARD instead of the
        # next forward; identical arithmetic, only the start time on the GPU moves
        self.early = False
        self._upload_done = None
        self._opt_stream = None
        self._seg_blocks = None
        self._events = None
        # exponential moving average of the weights (enable_ema): a flat fp32 buffer with the offsets of the weights that every update
        # launch moves along (crct_adamw_step_ema).  ``ema_decay`` is a plain attribute read at every step(): a decay schedule is the
        # caller's one line.  Under a GradScaler a skipped step leaves the average alone (decided on the device), but a host-side
        # schedule that counts step() calls counts the skipped ones too.
        self._ema = None
        self.ema_decay = 0.999
        self._ema_weight = 0.0
        self._ema_swapped = False
        # expose the moments the way torch.optim.AdamW does (views of the flat buffers)
        for e in self._segs:
            p = byname[e.name]
            self.state[p] = dict(step=torch.tensor(0.0), exp_avg=self._m[e.offset:e.offset + e.numel].view(e.shape),
                                 exp_avg_sq=self._v[e.offset:e.offset + e.numel].view(e.shape))
        self._byname = byname

    def _index_optional(self, blk_seg):
        opt_names = {e.name for e in getattr(self.core, "optional_entries", ())}
        self._opt_blocks = []
        for i, e in enumerate(self._segs):
            if e.name in opt_names:
                idx = (blk_seg == i).nonzero().flatten()
                if idx.numel():
                    self._opt_blocks.append((int(idx.min()), int(idx.max()) + 1, e))

    def _sync_active(self):
        """Follow the model's set of tensors without gradient: the block table on the device then holds exactly the segments whose
        Parameter has a gradient.  Host work only, and only when the set has changed."""
        core = self.core
        ver = getattr(core, "_nograd_version", 0)
        if ver == self._active_ver:
            return
        self._active_ver = ver
        nograd = core.tensors_without_grad
        dev = core.flat_params.device
        blk_seg, blk_off = active_blocks(self._blk_full[0], self._blk_full[1], [e.name not in nograd for e in self._segs])
        self._blk_prev = (self._blk_seg, self._blk_off)      # an overlapped update of the last step may still be reading them
        self._blk_seg, self._blk_off = blk_seg.to(dev), blk_off.to(dev)
        self._index_optional(blk_seg)
        self._seg_blocks = None                      # the overlap plan and launch groups are cut from the block table
        self._groups_key = None
        self._clip = None

    def covers_every_gradient(self):
        """Does this optimizer update every tensor that receives a gradient?  (One built over a parameter subset leaves the rest to
        somebody who reads ``.grad``.)"""
        nograd = getattr(self.core, "tensors_without_grad", ())
        return all(e.name in self._group_of or e.name in nograd for e in self._used)

    def set_early(self, on=True):
        """Overlap the update with the rest of backward (needs ``overlap``); see ``early`` above."""
        if on and getattr(self.core, "lm_loss_coeff", 0.0) > 0.0:
            # the masked-LM head's gradients are written by its own node in front of the engine's pass, whose segment events the early
            # update waits for: not built
            raise RuntimeError("FusedAdamW.set_early(True) with params['lm_loss_coeff'] > 0 is not supported: use the overlapped update "
                               "(overlap = True) without early mode")
        if on and getattr(self.core, "img_loss_coeff", 0.0) > 0.0:      # the masked-region head: the same node-in-front-of-the-pass order
            raise RuntimeError("FusedAdamW.set_early(True) with params['img_loss_coeff'] > 0 is not supported: use the overlapped update "
                               "(overlap = True) without early mode")
        self.early = bool(on)
        self.core.record_segment_events = bool(on)

    def _upload_hyper(self, stream=None):
        lrs = [self.param_groups[self._group_of[e.name]]["lr"] for e in self._segs]
        wds = [self.param_groups[self._group_of[e.name]]["weight_decay"] for e in self._segs]
        key = (tuple(lrs), tuple(wds))
        if key != self._last:
            if self._upload_done is not None:
                self._upload_done.synchronize()              # the pinned staging buffers are free again (long done in practice)
            self._lr_host.copy_(torch.tensor(lrs, dtype=torch.float32))
            self._wd_host.copy_(torch.tensor(wds, dtype=torch.float32))
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                self._lr_dev.copy_(self._lr_host, non_blocking=True)
                self._wd_dev.copy_(self._wd_host, non_blocking=True)
                if self._upload_done is None:
                    self._upload_done = torch.cuda.Event()
                self._upload_done.record()
            self._last = key

    def _launch(self, b0, b1, inv_scale, stream, max_workgroups=0):
        core, g0 = self.core, self.param_groups[0]
        if b1 <= b0:                 # nothing in this range has a gradient
            return
        frozen = [] if getattr(core, "optional_grads_live", True) else [e for lo, hi, e in self._opt_blocks if lo < b1 and hi > b0]
        if frozen:               # areas_emp without a gradient: its weights, moments and shadow are put back behind the update
            side = torch.cuda.ExternalStream(stream, device=core.flat_params.device)
            bufs = (core.flat_params, self._m, self._v, core.flat_shadow) + ((self._ema,) if self._ema is not None else ())
            with torch.cuda.stream(side):
                kept = [(e, [b[e.offset:e.offset + e.numel].clone() for b in bufs]) for e in frozen]
        args = (core.flat_params.data_ptr(), core.flat_grads.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                core.flat_shadow.data_ptr(), self._seg_off.data_ptr(), self._seg_len.data_ptr(),
                self._lr_dev.data_ptr(), self._wd_dev.data_ptr(), self._blk_seg.data_ptr() + 4 * b0,
                self._blk_off.data_ptr() + 8 * b0, b1 - b0, g0["betas"][0], g0["betas"][1], g0["eps"],
                max(self._step, 1), L.ptr(inv_scale), self._amp_arg, self._fp8_arg(), int(max_workgroups),
                int(self.fuse_zero_grad), L.ptr(self._g16))
        if self._ema is None:
            L.check(L.load().crct_adamw_step(*args, stream), "adamw_step")
        else:            # the average of the weights moves in the same launch (enable_ema)
            L.check(L.load().crct_adamw_step_ema(*args, self._ema.data_ptr(), self._ema_weight, stream), "adamw_step_ema")
        if frozen:
            with torch.cuda.stream(side):
                for e, saved in kept:
                    for b, v in zip(bufs, saved):
                        b[e.offset:e.offset + e.numel].copy_(v)

    # ---- torch.amp.GradScaler (train.py:157,208-212).  ``scaler.step(optimizer)`` sees ``_step_supports_amp_scaling`` and
    # hands over ``optimizer.grad_scale`` / ``optimizer.found_inf`` (device scalars) instead of unscaling 524 gradient views
    # itself; the update kernel divides by the scale, skips the step on inf / nan and takes its bias corrections from a
    # device-side step counter that only advances on real steps -- no host sync anywhere.
    _step_supports_amp_scaling = True

    def _amp_begin(self):
        import ctypes as C
        scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if scale is None and found is None:
            if self._step_dev is not None:                      # scaler went away: back to the host counter
                self._step = int(self._step_dev.item())
                self._step_dev = None
            self._amp_arg = None
            return False
        dev = self.core.flat_params.device
        if self._step_dev is None:
            self._step_dev = torch.tensor([self._step], dtype=torch.int32, device=dev)
        found32 = found.to(device=dev, dtype=torch.float32).reshape(1) if found is not None else None
        scale32 = scale.to(device=dev, dtype=torch.float32).reshape(1) if scale is not None else None
        L.check(L.load().crct_adamw_advance(self._step_dev.data_ptr(), L.ptr(found32), L.current_stream()), "adamw_advance")
        st = L.AmpState()
        st.grad_scale, st.found_inf, st.step = L.ptr(scale32), L.ptr(found32), self._step_dev.data_ptr()
        self._amp_keep = (scale32, found32, st)
        self._amp_arg = C.byref(st)
        return True

    def _fp8_state(self):
        """The model's Fp8State (crct/fp8.py) where there is an e4m3 weight shadow to maintain, else None."""
        st = getattr(self.core, "_fp8", None) if getattr(self.core, "fp8", False) else None
        return st if st is not None and st.weights else None

    def _fp8_arg(self):
        """CrctFp8Shadow of the model's e4m3 weight shadow (None unless the model runs the fp8 forward)."""
        st = self._fp8_state()
        return st.shadow_for(self._segs)[0] if st is not None else None

    @property
    def _fp8_transposes(self):
        """Does the update kernel itself keep the transposed shadow current?"""
        st = self._fp8_state()
        return st is not None and st.shadow_for(self._segs)[1]

    def _fp8_before_update(self, stream):
        """Delayed scaling of the weight shadow: the scales this update quantises with come from the amax the previous update saw
        (a step the GradScaler skips leaves shadow AND scales alone)."""
        if self._fp8_arg() is not None:     # (builds the descriptor: an optimizer that misses a shadowed weight is refused before any launch)
            self.core._fp8.weight.update(stream, skip_if=self._amp_keep[1] if (self._amp_arg is not None and self._amp_keep is not None) else None)

    def _launch_groups(self, order):
        """``order`` (segments in first-use order) cut into ``launch_groups`` runs of similar block counts, the first segment alone."""
        key = (tuple(order), self.launch_groups)
        if getattr(self, "_groups_key", None) != key:
            sizes = [self._seg_blocks[i][1] - self._seg_blocks[i][0] for i in order]
            groups, rest = [[order[0]]], order[1:]
            n_rest = max(self.launch_groups - 1, 1)
            target = (sum(sizes[1:]) + n_rest - 1) // n_rest
            cur, acc = [], 0
            for i, sz in zip(rest, sizes[1:]):
                cur.append(i)
                acc += sz
                if acc >= target and len(groups) < self.launch_groups - 1:
                    groups.append(cur)
                    cur, acc = [], 0
            if cur:
                groups.append(cur)
            for g in groups:                     # block ranges of a run must be adjacent (the flat buffer is in reverse first-use order)
                spans = sorted(self._seg_blocks[i] for i in g if self._seg_blocks[i][1] > self._seg_blocks[i][0])
                if any(a[1] != b[0] for a, b in zip(spans, spans[1:])):
                    raise RuntimeError("optimizer launch groups: segments of a group are not adjacent in the block table")
            self._groups_key, self._groups = key, groups
            self._group_events = [None] * len(self._seg_blocks)
        return self._groups

    def _plan_overlap(self):
        """Block ranges of the optimizer's table per engine backward-segment (both are sorted by flat offset)."""
        eng = self.core._engine
        if eng is None:
            return False
        import bisect
        blk_seg = self._blk_seg.cpu().tolist()
        offs = [e.offset for e in self._segs]
        self._seg_blocks = []
        for lo, hi in eng.segments:
            s0, s1 = bisect.bisect_left(offs, lo), bisect.bisect_left(offs, hi)
            # blocks are in segment order: the first block of the first segment >= s that has any (segments without gradient have none)
            self._seg_blocks.append((bisect.bisect_left(blk_seg, s0), bisect.bisect_left(blk_seg, s1)))
        covered = sum(b1 - b0 for b0, b1 in self._seg_blocks)
        if covered != len(blk_seg):
            raise RuntimeError("optimizer overlap plan does not cover every block (%d of %d)" % (covered, len(blk_seg)))
        self._opt_stream = self.core.aux_stream()        # shared with the data-parallel exchange (crct/ddp.py)
        from .events import DeviceEvent
        self._events = [DeviceEvent() for _ in eng.segments]
        return True

    def _follow_device(self):
        """The model was moved (``model.to('cuda:1')`` after the optimizer was built): the moments and tables follow, and
        everything bound to the old device -- update stream, segment events -- is made again (the fp8 shadow descriptor lives
        in the model's Fp8State, which the move has dropped)."""
        dev = self.core.flat_params.device
        if self._m.device == dev:
            return
        old_m, old_v = self._m, self._v
        self._m, self._v = old_m.to(dev), old_v.to(dev)
        if self._ema is not None:
            self._ema = self._ema.to(dev)
        for e in self._segs:
            st = self.state[self._byname[e.name]]
            st["exp_avg"] = self._m[e.offset:e.offset + e.numel].view(e.shape)
            st["exp_avg_sq"] = self._v[e.offset:e.offset + e.numel].view(e.shape)
        for k in ("_seg_off", "_seg_len", "_blk_seg", "_blk_off", "_lr_dev", "_wd_dev"):
            setattr(self, k, getattr(self, k).to(dev))
        self._last = None
        self._upload_done = None
        self._events = self._opt_stream = self._seg_blocks = None
        self._clip = self._clip_partials = self._clip_seg_norms = self._clip_keep = None
        self._step_dev = self._step_dev.to(dev) if self._step_dev is not None else None

    @torch.no_grad()
    def step(self, closure=None, inv_scale=None):
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.step() inside swap_ema(): the weights are the averaged ones; leave the context first")
        loss = closure() if closure is not None else None
        core = self.core
        self._follow_device()
        if self._ema is not None:
            self._ema_weight = float(np.float32(1.0 - float(self.ema_decay)))
        self._sync_active()
        amp = self._amp_begin()
        if not amp:
            self._step += 1
        # data-parallel bf16 exchange: the all-reduced gradients live in the communication buffer (crct/ddp.py), not in .grad
        ddp = getattr(core, "_ddp", None)
        self._g16 = ddp.grad_source() if ddp is not None else None
        if self._g16 is not None and (amp or inv_scale is not None):
            raise RuntimeError("GradScaler / unscaling reads the fp32 .grad views: construct FlatGradDDP(..., materialize_grads=True) "
                               "(or grad_dtype=torch.float32) when training with a GradScaler")
        inv_scale = self._take_clip_coefficient(inv_scale)
        if self.overlap and not amp and (self._seg_blocks is not None or self._plan_overlap()):
            cur = torch.cuda.current_stream()
            self._opt_stream = core.aux_stream()          # the engine's auxiliary stream (re-fetched: an engine rebuilt for a larger batch has new streams)
            done = None
            if self.early and inv_scale is None:
                done = core.take_segment_done_events()
                if done is None and ddp is not None and ddp.last_exchange is not None:
                    done = ddp.segment_waits()       # AdamW of a bucket behind THAT bucket's all-reduce, not behind all of them
            n = len(self._seg_blocks)
            if done is None:
                self._upload_hyper()
                # gradients (and the hyper-parameter upload) are final; after an all-reduce across GPUs they were written by
                # peer devices: system-scope ordering then
                ddp = getattr(core, "_ddp", None)
                order_streams(cur, self._opt_stream, system=ddp is not None and getattr(ddp, "world", 1) > 1)
                order = range(n - 1, -1, -1)                  # first-use order: embeddings ... heads
            else:
                self._upload_hyper(self._opt_stream)          # not behind the backward pass that `cur` still runs
                order = range(n)                              # the order backward finishes them: heads ... embeddings
            self._fp8_before_update(self._opt_stream.cuda_stream)
            if done is None and self.launch_groups > 0:
                # fewer, larger launches: consecutive segments (adjacent block ranges) share one launch and one event; the first
                # group is the first segment alone, so that the next forward can start at once
                for members in self._launch_groups(list(order)):
                    b0 = min(self._seg_blocks[i][0] for i in members)
                    b1 = max(self._seg_blocks[i][1] for i in members)
                    if b1 > b0:
                        self._launch(b0, b1, inv_scale, self._opt_stream.cuda_stream, self.overlap_workgroups)
                    ev = self._events[members[0]]
                    ev.record(self._opt_stream)
                    for i in members[1:]:
                        self._group_events[i] = ev
                    self._group_events[members[0]] = ev
                core._param_events = list(self._group_events)
                core._opt_stream = self._opt_stream
                order = ()
            launched = 0
            for sgi in order:
                b0, b1 = self._seg_blocks[sgi]
                if done is not None:
                    for w in done[sgi]:
                        w(self._opt_stream)
                if b1 > b0:
                    # the first launches in first-use order (embeddings, first layers) run while the next forward is still waiting
                    # for them: nothing to share the chip with yet, so no throttle (full_width_first = how many)
                    wide = done is None and launched < int(self.full_width_first)
                    self._launch(b0, b1, inv_scale, self._opt_stream.cuda_stream, 0 if wide else self.overlap_workgroups)
                    launched += 1
                self._events[sgi].record(self._opt_stream)
            if done is not None:
                order_streams(cur, self._opt_stream)          # the gradient memset that follows must not pass backward's tail
            if not (done is None and self.launch_groups > 0):
                core._param_events = self._events            # the next forward waits segment by segment
            core._opt_stream = self._opt_stream               # ... and the next backward for the whole stream
        else:
            self._upload_hyper()
            self._fp8_before_update(L.current_stream())
            self._launch(0, self._blk_seg.numel(), inv_scale, L.current_stream())
        st = self._fp8_state()
        if st is not None:                              # transposed shadow and gradient scales follow the update on the same stream
            beside = self.overlap and not amp and self._opt_stream is not None
            st.after_update(self._opt_stream.cuda_stream if beside else L.current_stream(), self._fp8_transposes,
                            self.fp8_transpose_workgroups if beside else 0)
        core.note_params_updated_natively()
        # under GradScaler the kernel returns at once on a skipped step and zeroes nothing: only without it the clear is certain
        self._grads_cleared = bool(self.fuse_zero_grad) and not amp
        if self._grads_cleared:
            core._grads_dirty = False                         # until the next backward pass
        return loss

    # ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ on the flat buffers)
    def _grad_buffer(self):
        """The buffer the next step() reads its gradients from: the data-parallel exchange's bf16 buffer, else the fp32 one."""
        ddp = getattr(self.core, "_ddp", None)
        g16 = ddp.grad_source() if ddp is not None else None
        return g16 if g16 is not None else self.core.flat_grads

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type=2.0, error_if_nonfinite=False, grad_scaler=None, in_place=False):
        """``torch.nn.utils.clip_grad_norm_`` over every gradient this optimizer updates: one streaming pass over the buffer the
        next ``step()`` reads (the bf16 exchange buffer of ``FlatGradDDP`` when that holds the reduced gradients, else the flat
        fp32 one) and one small launch.  Returns the total norm as a 0-d device tensor; nothing waits for the GPU unless
        ``error_if_nonfinite`` is set.  Call it after ``backward()`` and before ``step()``.

        By default NOTHING IS RESCALED: ``.grad`` keeps the unclipped values, and the clip coefficient (a device scalar) is
        multiplied into the gradients inside the update kernel by exactly the next ``step()``; that ``step()`` and ``zero_grad()``
        drop it.  ``in_place=True`` multiplies the fp32 gradient buffer now instead, for callers that read ``.grad`` afterwards
        (refused while the gradients live in the bf16 exchange buffer: the fp32 views of the Linear weights are NaN there).

        ``grad_scaler``: the ``torch.amp.GradScaler`` whose factor is still on the gradients (the call sits between
        ``scaler.scale(loss).backward()`` and ``scaler.step(optimizer)``, without ``scaler.unscale_``): the norm returned and
        compared with ``max_norm`` is then the norm of the unscaled gradients.  ``norm_type``: 2 or ``inf``.
        ``max_norm=float('inf')`` never clips: a cheap gradient-health probe (see ``grad_norms()``)."""
        norm_type = float(norm_type)
        if norm_type == 2.0:
            kind = 0
        elif norm_type == float("inf"):
            kind = 1
        else:
            raise ValueError("clip_grad_norm_: norm_type must be 2 or inf (got %r)" % (norm_type,))
        if self.early:
            raise RuntimeError("clip_grad_norm_: in early mode the update of a segment starts before the last gradient exists, so a "
                               "global norm cannot be applied; call set_early(False)")
        self._follow_device()
        self._sync_active()
        core = self.core
        src = self._grad_buffer()
        if in_place and src is not core.flat_grads:
            raise ValueError("clip_grad_norm_(in_place=True) rescales the fp32 .grad views, which do not hold the exchanged bf16 "
                             "gradients: use the default (deferred) mode, or construct FlatGradDDP(..., materialize_grads=True)")
        scale = None
        if grad_scaler is not None and grad_scaler.is_enabled():
            scale = grad_scaler._get_scale_async()
            if scale is None:
                raise RuntimeError("clip_grad_norm_(grad_scaler=...): the scaler has not scaled a loss yet; call it between "
                                   "scaler.scale(loss).backward() and scaler.step(optimizer)")
            scale = scale.to(device=src.device, dtype=torch.float32).reshape(1)
        if self._clip_partials is None or self._clip_partials.numel() != self._blk_seg.numel():
            self._clip_partials = torch.empty(self._blk_seg.numel(), dtype=torch.float32, device=src.device)
        ops.grad_sumsq(src, self._seg_off, self._seg_len, self._blk_seg, self._blk_off, partials=self._clip_partials, norm_kind=kind)
        out, per = ops.grad_norm_finalize(self._clip_partials, self._blk_seg, len(self._segs), max_norm, norm_kind=kind, grad_scale=scale)
        self._clip_seg_norms = per
        self._clip = None
        if in_place:
            ops.scale_runs(core.flat_grads, out[1:2], self._seg_off, self._seg_len, self._blk_seg, self._blk_off)
        else:
            self._clip = dict(out=out, kind=kind, max_norm=float(max_norm), scale=scale)
        self._clip_keep = (out, scale)          # alive until the kernels that read them have been launched
        if error_if_nonfinite and not bool(torch.isfinite(out[0])):
            self._clip = None
            raise RuntimeError("The total norm of order %s for gradients is non-finite, so it cannot be clipped" % norm_type)
        return out[0]

    def _take_clip_coefficient(self, inv_scale):
        """The ``inv_scale_dev`` argument of this step's launches: the pending clip coefficient (consumed here), times the caller's
        ``inv_scale`` where both exist (the finalize launch again, over the partials it kept)."""
        clip, self._clip = self._clip, None
        if clip is None:
            return inv_scale
        if inv_scale is None:
            coef = clip["out"][1:2]
        else:
            mul = inv_scale.to(device=self._clip_partials.device, dtype=torch.float32).reshape(1)
            out, _ = ops.grad_norm_finalize(self._clip_partials, self._blk_seg, len(self._segs), clip["max_norm"], norm_kind=clip["kind"],
                                            grad_scale=clip["scale"], mul=mul, seg_norm=False)
            coef = out[1:2]
        self._clip_keep = (clip["out"], clip["scale"], coef)
        return coef

    def grad_norms(self):
        """Per-tensor gradient norms of the last ``clip_grad_norm_`` pass (its ``norm_type``, unscaled like its result): fp32 device
        tensor ``[len(grad_norm_names)]``; None before the first pass."""
        return self._clip_seg_norms

    @property
    def grad_norm_names(self):
        """State-dict keys of the tensors ``grad_norms()`` lists, in its order."""
        return [e.name for e in self._segs]

    def synchronize(self):
        """Order the current stream after an in-flight overlapped update (before reading weights outside forward)."""
        if self._opt_stream is not None:
            order_streams(self._opt_stream, torch.cuda.current_stream())

    # ---- exponential moving average of the weights, kept by the update launches themselves
    @property
    def ema_enabled(self):
        return self._ema is not None

    @torch.no_grad()
    def enable_ema(self, decay=0.999):
        """Keep an exponential moving average of the weights: ``ema += (1 - ema_decay) * (w_new - ema)`` for every element an update
        launch writes, inside that launch -- it follows the overlap / early streams, a GradScaler's skipped steps and the frozen
        tensors without a host sync or a launch of its own (4 B read + 4 B written per parameter).  The buffer (the size of the fp32
        weights) starts as a copy of the current weights, so tensors no update ever touches read as their weights for ever."""
        if self._ema_swapped:
            raise RuntimeError("enable_ema() inside swap_ema()")
        self._follow_device()
        self.ema_decay = decay
        self._ema = torch.zeros_like(self.core.flat_params)
        self.ema_reset()

    def disable_ema(self):
        """Stop averaging and free the buffer."""
        if self._ema_swapped:
            raise RuntimeError("disable_ema() inside swap_ema()")
        self.synchronize()
        self._ema = None

    @torch.no_grad()
    def ema_reset(self):
        """The average := the current weights (after ``load_state_dict`` on the model, or to restart the average)."""
        self._need_ema()
        self._follow_device()
        self.synchronize()
        self._ema.copy_(self.core.flat_params)

    def _need_ema(self):
        if self._ema is None:
            raise RuntimeError("the weight average is off: call enable_ema() first")

    def _ema_keys(self, model=None):
        """(state-dict key, table entry) in the order of ``model.state_dict()``: every table entry under the key that model gives it
        (``bert_pretrained.`` in front for the VisualDialogEncoder wrapper), and the tied decoder weight under its second key.
        ``model``: the model the optimizer was built for, unless given."""
        model = model if model is not None else self._model_ref()
        prefix = ""
        if model is not None and model is not self.core and hasattr(model, "named_modules"):
            for name, mod in model.named_modules():
                if mod is self.core:
                    prefix = name + "."
        by = {e.name: e for e in self.core.table}
        tied = {"cls.predictions.decoder.weight": "bert.embeddings.word_embeddings.weight"}
        return [(prefix + k, by[tied.get(k, k)]) for k in self.core.state_dict().keys()]

    @torch.no_grad()
    def ema_state_dict(self, model=None):
        """``{name: tensor}`` of the averaged weights with the keys, shapes and order of ``model.state_dict()`` (the model the optimizer
        was built for, or the wrapper / core model given): independent copies, the tied ``cls.predictions.decoder.weight`` included as
        the model's own state dict includes it; loads into any such model with ``load_state_dict``."""
        self._need_ema()
        self.synchronize()
        src = self.core.flat_params if self._ema_swapped else self._ema
        return {k: src[e.offset:e.offset + e.numel].view(e.shape).clone() for k, e in self._ema_keys(model)}

    @torch.no_grad()
    def load_ema_state_dict(self, sd, model=None):
        """The reverse of ``ema_state_dict`` by key intersection; returns the number of tensors taken."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("load_ema_state_dict() inside swap_ema()")
        self._follow_device()
        self.synchronize()
        n = 0
        for k, e in self._ema_keys(model):
            if k in sd:
                self._ema[e.offset:e.offset + e.numel].view(e.shape).copy_(sd[k])
                n += 1
        return n

    @torch.no_grad()
    def _exchange_with_ema(self):
        """flat weights <-> average, through a bounded staging buffer"""
        p, a = self.core.flat_params, self._ema
        piece = 1 << 26
        for o in range(0, p.numel(), piece):
            t = p[o:o + piece].clone()
            p[o:o + piece].copy_(a[o:o + piece])
            a[o:o + piece].copy_(t)

    @contextlib.contextmanager
    def swap_ema(self):
        """``with optimizer.swap_ema(): evaluate(model)`` -- inside, the model's weights ARE the averaged ones (the flat weights and the
        average exchange contents; the bf16 shadow, and with fp8 the e4m3 shadows and their scales, are rebuilt from them by the next
        forward).  On exit the training weights come back together with the shadows and fp8 scale state exactly as the last update left
        them: the next training step is bit-identical to one of a run that never swapped.  ``step()`` inside, and nesting, raise."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("swap_ema() is already active (it does not nest)")
        core = self.core
        self._follow_device()
        self.synchronize()
        # what the updates have written beside the weights: restored bit for bit, not recomputed (the fp8 weight scales are DELAYED
        # ones, which a requantisation from the weights would replace by exact ones)
        saved_b16 = core.flat_shadow.clone() if core._shadow_ver == core._param_version() else None
        st = getattr(core, "_fp8", None)
        saved_f8 = None
        if st is not None:
            sets = (st.weight, st.act, st.grad)
            saved_f8 = (st.q.clone(), st.qt.clone() if st.qt is not None else None,
                        [(x.scale.clone(), x.amax.clone(), x.updates) for x in sets],
                        (st.calibrated, st.scaled, st.bwd_calibrated, st.g_scales_fresh))
        self._exchange_with_ema()
        core._invalidate_shadow()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange_with_ema()
            self._ema_swapped = False
            if saved_b16 is not None:
                core.flat_shadow.copy_(saved_b16)
                core.note_params_updated_natively()
            else:
                core._invalidate_shadow()
            if saved_f8 is not None and getattr(core, "_fp8", None) is st:
                st.q.copy_(saved_f8[0])
                if st.qt is not None:
                    st.qt.copy_(saved_f8[1])
                for x, (sc, am, n) in zip((st.weight, st.act, st.grad), saved_f8[2]):
                    x.scale.copy_(sc)
                    x.amax.copy_(am)
                    x.updates = n
                st.calibrated, st.scaled, st.bwd_calibrated, st.g_scales_fresh = saved_f8[3]
            elif getattr(core, "_fp8", None) is not None:     # the fp8 state was made inside the context, from the averaged weights:
                core._fp8.requantize(core.flat_params, L.current_stream())      # start-up quantisation again, from the training weights

    def zero_grad(self, set_to_none=True):
        # one memset; .grad views stay attached (set_to_none would only force a re-attach next step)
        self._clip = None                                     # a clip coefficient belongs to the gradients it was computed from
        if getattr(self, "_grads_cleared", False) and not self.core._grads_dirty:
            return                                            # step() has already zeroed them (fuse_zero_grad)
        if self.overlap and self._opt_stream is not None:
            with torch.cuda.stream(self._opt_stream):        # after the update that is still reading the gradients
                self.core.zero_flat_grads(lazy=self.lazy_zero_grad)
        else:
            self.core.zero_flat_grads(lazy=self.lazy_zero_grad)

    def state_dict(self):
        if self._step_dev is not None:
            self._step = int(self._step_dev.item())
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        idx = 0
        pos_to_param = {}
        for g, sg in zip(self.param_groups, groups):
            for p, sid in zip(g["params"], sg["params"]):
                pos_to_param[sid] = p
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        step = 0
        for sid, st in state_dict["state"].items():
            p = pos_to_param[sid]
            mine = self.state.get(p)
            if mine is None:
                continue
            mine["exp_avg"].copy_(st["exp_avg"])
            mine["exp_avg_sq"].copy_(st["exp_avg_sq"])
            step = max(step, int(float(st["step"])))
        self._step = step
        self._step_dev = None
        self._last = None


def clip_grad_norm_(model_or_optimizer, max_norm, **kw):
    """``torch.nn.utils.clip_grad_norm_`` for a model trained by ``FusedAdamW``: finds the optimizer attached to the model (or
    takes the optimizer itself, or a ``FlatGradDDP`` wrapper) and calls its ``clip_grad_norm_``; see there for the keywords and
    for what happens to ``.grad`` (nothing, by default)."""
    opt = model_or_optimizer
    if not isinstance(opt, FusedAdamW):
        ref = getattr(_crct_core(model_or_optimizer), "_fused_optimizer", None)
        opt = ref() if callable(ref) else None
        if opt is None:
            raise RuntimeError("clip_grad_norm_: no live FusedAdamW is attached to this model (crct.optim.get_optimizer builds one)")
    return opt.clip_grad_norm_(max_norm, **kw)


def get_optimizer(params, dialog_encoder, language_weights_json=None):
    """utils.py:228-249 with the fused kernel underneath.  ``language_weights_json`` may point at the
    reference's ``config/language_weights.json``; by default its membership rule is applied
    (crct.layout.is_language_weight)."""
    listed = None
    path = language_weights_json or os.path.join("config", "language_weights.json")
    if language_weights_json or os.path.exists(path):
        with open(path) as f:
            listed = set(json.load(f))
    groups = []
    for key, value in dict(dialog_encoder.named_parameters()).items():
        if not value.requires_grad:
            continue
        bare = key[len("bert_pretrained."):] if key.startswith("bert_pretrained.") else key
        lang = (key in listed) if listed is not None else is_language_weight(bare)
        lr = params["lr"] if lang else params["image_lr"]
        wd = 0 if any(nd in key for nd in NO_DECAY) else params["wd"]
        groups.append({"params": [value], "lr": lr, "weight_decay": wd})
    return FusedAdamW(groups, dialog_encoder, lr=params["lr"])
