"""Host-side state of the fp8 step (params['fp8'], BASELINE configs[4]): the e4m3 weight shadow and its transposed copy, the three
families of delayed scales (activations, gradients, weights) and the protocol that decides which pass calibrates, which updates scales
and which quantises.  ``CrctModel._fp8`` is one ``Fp8State`` (or None); the fused AdamW reaches the same object through the model.

The decisions are pure functions of offsets and flags -- ``tile_table``, ``segment_shadow_map``, ``forward_plan``, ``backward_plan``,
``next_reset`` -- and the methods of ``Fp8State`` / ``ScaleSet`` are thin drivers that turn them into library calls."""
import bisect
import ctypes as C

import torch

from . import lib as L
from . import ops

AMAX_WINDOW = 256          # calls between resets of a scale family's running maxima (see crct_fp8_update_scales)
E4M3_MAX, E5M2_MAX = 448.0, 57344.0


# ------------------------------------------------------------------------------------------- pure functions
def next_reset(count, window=AMAX_WINDOW):
    """(count + 1, reset) of a scale family's update counter: the counter moves first, every ``window``-th call resets the maxima."""
    count += 1
    return count, int(count % window == 0)


def tile_table(weights, w_in):
    """64 x 64 tile table of crct_fp8_transpose_weights over ``weights`` = [(offset, numel)] stored [out][in]: first tile of each
    weight and the tile count.  Every shadowed weight has a transposed copy (a fused QKV weight [3H][H] is one of them)."""
    begins, nt = [], 0
    for (_, num), n_in in zip(weights, w_in):
        begins.append(nt)
        nt += ((num // n_in + 63) // 64) * ((n_in + 63) // 64)
    return begins, nt


def segment_shadow_map(weights, w_in, segs, have_qt):
    """Optimizer segments ``segs`` = [(offset, numel)] onto the shadow slots ``weights`` = [(offset, numel)] (in the engine's model
    order, not sorted by offset) -> (slots, t_in, t_base, t_ld, fused).  AdamW segments are parameter tensors: a fused QKV weight spans
    three.  slots[s] = the weight segment s lies in, or -1.  The transposed shadow is kept by the update itself, in whole 64 x 64
    tiles, where the segment is a band of whole rows of the weight (the weight itself, or the Q / K / V part of a fused QKV weight):
    t_in / t_base / t_ld are then the weight's ``in``, the band's first byte in the transposed copy and that copy's leading dimension,
    else 0.  ``fused``: every weight is covered by such bands, so no separate crct_fp8_transpose_weights launch is needed."""
    by_start = sorted(range(len(weights)), key=lambda i: weights[i][0])
    starts = [weights[i][0] for i in by_start]
    slots, t_in, t_base, t_ld = [], [], [], []
    for off, numel in segs:
        k = bisect.bisect_right(starts, off) - 1
        k = by_start[k] if k >= 0 else -1
        inside = k >= 0 and off + numel <= weights[k][0] + weights[k][1]
        slots.append(k if inside else -1)
        ok = inside and have_qt
        if ok:
            w_off, n_in = weights[k][0], w_in[k]
            ok = n_in % 64 == 0 and (off - w_off) % n_in == 0 and numel % (64 * n_in) == 0 and ((off - w_off) // n_in) % 16 == 0
        t_in.append(w_in[k] if ok else 0)
        t_base.append(weights[k][0] + (off - weights[k][0]) // w_in[k] if ok else 0)
        t_ld.append(weights[k][1] // w_in[k] if ok else 0)
    hit = set(s for s in slots if s >= 0)
    if hit != set(range(len(weights))):
        raise RuntimeError("fused AdamW: %d of the model's %d fp8-shadowed weights are not covered by optimizer segments; their "
                           "shadow would go stale" % (len(weights) - len(hit), len(weights)))
    covered = [0] * len(weights)
    for s, t, (_, numel) in zip(slots, t_in, segs):
        if s >= 0 and t > 0:
            covered[s] += numel
    fused = bool(have_qt) and all(covered[k] == weights[k][1] for k in range(len(weights)))
    return slots, t_in, t_base, t_ld, fused


def forward_plan(fp8_forward, fp8_wgrad, train_grad, training, calibrated, scaled):
    """What an fp8 model's forward does -> (pass_args, dry_pass, update_act, fp8_mode, backward_only).

    Neither fp8 forward nor fp8 weight gradients = fp8 DATA GRADIENTS only: nothing of the forward pass is quantised (no e4m3 copies,
    no activation maxima), the state is handed over only where a backward pass follows (``train_grad``).  Otherwise the first forward
    runs one dry pass that collects every activation amax (bf16 GEMMs), the activation scales move on in training and once before the
    first evaluation pass (delayed scaling: a pass quantises with the previous pass's amax), and ``fp8_mode`` 2 keeps the forward
    GEMMs on bf16 operands while the e4m3 copies / maxima the fp8 backward reads are still written."""
    if not fp8_forward and not fp8_wgrad:
        return bool(train_grad), False, False, 1, True
    return True, not calibrated, bool(training or not scaled), 1 if fp8_forward else 2, False


def backward_plan(bwd_calibrated, g_scales_fresh):
    """(mode, update_grad_scales_first) of an fp8 backward pass: the first pass only collects the gradient maxima (mode 2, its GEMMs
    run in bf16), from then on the e5m2 copies are quantised with the scales of the previous passes (mode 1) -- refreshed here first
    unless the optimizer has done so on its stream."""
    mode = 1 if bwd_calibrated else 2
    return mode, mode == 1 and not g_scales_fresh


# ------------------------------------------------------------------------------------------- device state
class ScaleSet:
    """One family of delayed scales: ``scale`` fp32 [n], ``amax`` fp32 [n * FP8_AMAX_LANES] (running maxima), the format's largest
    value ``fmax`` and the count of updates so far (the window is counted on the host per CALL)."""

    def __init__(self, n, fmax, device):
        self.n, self.fmax, self.updates, self.window = int(n), float(fmax), 0, AMAX_WINDOW
        self.scale = torch.ones(max(self.n, 1), device=device)
        self.amax = torch.zeros(max(self.n, 1) * L.FP8_AMAX_LANES, device=device)

    def update(self, stream, skip_if=None):
        """scale = fmax / amax from the running maxima, which are reset on every ``window``-th call; ``skip_if`` (device fp32 [1],
        a GradScaler's found_inf) leaves scales and maxima alone when set."""
        self.updates, reset = next_reset(self.updates, self.window)
        L.check(L.load().crct_fp8_update_scales(self.scale.data_ptr(), self.amax.data_ptr(), self.n, reset, L.ptr(skip_if), self.fmax, stream),
                "fp8_update_scales")


class Fp8State:
    """Device state of the fp8 step, created with the model's first engine: the e4m3 weight shadow ``q`` (same element offsets as the
    flat fp32 buffer) and its transposed copy ``qt`` (same byte offsets, every weight stored [in][out]; fp8 backward only), the scale
    families ``weight`` (one per shadowed weight), ``act`` (one per producer site) and ``grad`` (one per gradient site), the device
    tables of the quantise / transpose launches, and where the delayed-scaling protocol stands."""

    def __init__(self, table, total, device, engine, fp8_backward=True, fp8_wgrad=True, fp8_forward=True):
        self.fp8_backward, self.fp8_wgrad, self.fp8_forward = bool(fp8_backward), bool(fp8_wgrad), bool(fp8_forward)
        self.n_sites, self.weights = engine.fp8_layout()
        self.n_gsites = engine.lib.crct_engine_fp8_grad_sites(engine.handle)
        weights, dev = self.weights, device
        self.q = torch.zeros(total, dtype=torch.uint8, device=dev)
        self.qt = torch.zeros(total, dtype=torch.uint8, device=dev) if self.fp8_backward else None
        self.weight = ScaleSet(len(weights), E4M3_MAX, dev)
        self.act = ScaleSet(self.n_sites, E4M3_MAX, dev)
        self.grad = ScaleSet(self.n_gsites, E5M2_MAX, dev)
        # chunk table over the shadowed weights themselves (one segment per weight, slot = its index)
        lens = [n for _, n in weights]
        blk_seg, blk_off = ops.adamw_plan(lens) if lens else (torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64))
        self.seg_off = torch.tensor([o for o, _ in weights], dtype=torch.int64, device=dev)
        self.seg_len = torch.tensor(lens, dtype=torch.int64, device=dev)
        self.seg_slot = torch.arange(len(weights), dtype=torch.int32, device=dev)
        self.blk_seg, self.blk_off = blk_seg.to(dev), blk_off.to(dev)
        # transposed shadow: [out][in] of every weight and its 64 x 64 tiles
        by_off = {e.offset: e for e in table}
        self.w_in_host = [by_off[off].shape[1] for off, _ in weights]
        begins, self.n_tiles = tile_table(weights, self.w_in_host)
        self.w_out = torch.tensor([num // n_in for (_, num), n_in in zip(weights, self.w_in_host)], dtype=torch.int32, device=dev)
        self.w_in = torch.tensor(self.w_in_host, dtype=torch.int32, device=dev)
        self.tile_begin = torch.tensor(begins, dtype=torch.int64, device=dev)
        # protocol: activation maxima collected (dry pass) / activation scales set at least once; gradient maxima collected (first
        # backward) / gradient scales already refreshed for the next backward (by the optimizer)
        self.calibrated = self.scaled = self.bwd_calibrated = self.g_scales_fresh = False
        self._shadow = None

    # ---- weight shadow
    def requantize(self, flat_p, stream):
        """Exact per-tensor quantisation of the current fp32 weights (start-up, load_state_dict, foreign optimizers) and the
        transposed copy; the fused AdamW keeps both current by itself afterwards."""
        if not self.weights:
            return
        L.check(L.load().crct_fp8_quantize_weights(flat_p.data_ptr(), self.q.data_ptr(), self.seg_off.data_ptr(), self.seg_len.data_ptr(),
                                                   self.seg_slot.data_ptr(), self.blk_seg.data_ptr(), self.blk_off.data_ptr(),
                                                   self.blk_seg.numel(), self.weight.scale.data_ptr(), self.weight.amax.data_ptr(),
                                                   len(self.weights), stream), "fp8_quantize_weights")
        self.transpose(stream)

    def transpose(self, stream, max_workgroups=0):
        """The transposed e4m3 weight shadow the fp8 data-gradient GEMMs read, rebuilt from the shadow (one launch, 2 bytes per
        shadowed weight element)."""
        if self.qt is None or not self.weights:
            return
        L.check(L.load().crct_fp8_transpose_weights(self.q.data_ptr(), self.qt.data_ptr(), self.seg_off.data_ptr(), self.w_out.data_ptr(),
                                                    self.w_in.data_ptr(), self.tile_begin.data_ptr(), len(self.weights), self.n_tiles,
                                                    int(max_workgroups), stream), "fp8_transpose_weights")

    # ---- the step
    def forward_args(self):
        return (self.q, self.weight.scale, self.act.scale, self.act.amax)

    def begin_forward(self, step, train_grad, training, run_dry_pass):
        """The fp8 entries of a forward pass's ``step`` (see ``forward_plan``); ``run_dry_pass(step)`` runs the engine's forward.  The
        activation scales are updated on the current stream."""
        pass_args, dry_pass, update_act, fp8_mode, backward_only = forward_plan(self.fp8_forward, self.fp8_wgrad, train_grad, training,
                                                                                self.calibrated, self.scaled)
        if pass_args:
            step["fp8"] = self.forward_args()
        if backward_only:
            step["fp8_backward_only"] = True
        if dry_pass:
            run_dry_pass(dict(step, seg_events=None, fp8_mode=2))      # bf16 GEMMs, maxima only
            self.calibrated = True
        if update_act:
            self.act.update(L.current_stream())
            self.scaled = True
        if fp8_mode == 2:
            step["fp8_mode"] = 2

    def begin_backward(self, step, stream):
        """``step`` of a backward pass, with ``fp8_bwd`` where the pass has fp8 data gradients (see ``backward_plan``)."""
        if not self.fp8_backward or step.get("fp8") is None or self.n_gsites <= 0:
            return step
        mode, update_first = backward_plan(self.bwd_calibrated, self.g_scales_fresh)
        if update_first:
            self.update_grad_scales(stream)
        self.g_scales_fresh = False
        self.bwd_calibrated = True
        return dict(step, fp8_bwd=(mode, self.qt, self.grad.scale, self.grad.amax, self.fp8_wgrad))

    def update_grad_scales(self, stream):
        """Gradient scales from the maxima the last backward pass collected.  The fused AdamW does it on its own stream, off the
        critical path; without it the next backward pass does it first thing."""
        if self.fp8_backward and self.bwd_calibrated and self.n_gsites > 0:
            self.grad.update(stream)
            self.g_scales_fresh = True

    # ---- the fused AdamW
    def shadow_for(self, segs):
        """(CrctFp8Shadow argument of crct_adamw_step, does the update keep the transposed copy itself) for the optimizer segments
        ``segs`` (table entries); (None, False) without shadowed weights.  Built once per list: the descriptor and its tables live here."""
        if not self.weights:
            return None, False
        if self._shadow is None or self._shadow[0] is not segs:
            slots, t_in, t_base, t_ld, fused = segment_shadow_map(self.weights, self.w_in_host, [(e.offset, e.numel) for e in segs],
                                                                  self.qt is not None)
            dev = self.q.device
            tables = (torch.tensor(slots, dtype=torch.int32, device=dev), torch.tensor(t_in, dtype=torch.int32, device=dev),
                      torch.tensor(t_base, dtype=torch.int64, device=dev), torch.tensor(t_ld, dtype=torch.int32, device=dev))
            sh = L.Fp8Shadow()
            sh.q, sh.seg_slot, sh.scale, sh.amax = self.q.data_ptr(), tables[0].data_ptr(), self.weight.scale.data_ptr(), self.weight.amax.data_ptr()
            if fused:
                sh.qt, sh.seg_in, sh.seg_t_base, sh.seg_t_ld = self.qt.data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr()
            self._shadow = (segs, C.byref(sh), fused, sh, tables)
        return self._shadow[1], self._shadow[2]

    def after_update(self, stream, transposes_fused, workgroups=0):
        """Behind an optimizer update, on its stream: the update rewrote the e4m3 shadow, so its transposed copy follows (normally the
        update kernel has written it itself), then the scales the NEXT backward pass quantises its gradients with."""
        if not self.fp8_backward:
            return
        if not transposes_fused:
            self.transpose(stream, workgroups)
        self.update_grad_scales(stream)
