"""The fp8 state object (crct/fp8.py) on the GPU (-m gpu): the delayed-scaling protocol step by step, the library launches of each of its
phases, and the shadow descriptor of the fused AdamW.  One full-width model (vilbert_config, every dropout 0) at B = 3, T = 31, V = 7,
F_v = 2048 -- the smallest shape the fp8 kernels run at in this suite (test_fp8_mode_through_the_training_loop_paths) -- taken once
through: training forward, evaluation forward, backward, forward + backward, one FusedAdamW step, forward + backward.  No oracle run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402

# Library launches (crct_prof_enable(2): one stamp per kernel the library launches) of each phase.  Provenance: this module's _sequence run
# on the commit before crct/fp8.py existed (1f48e02), through an adapter that presented that commit's state dict under today's attribute
# names.  The refactor must not add, drop or move a launch.
#   train_fwd: shadow quantisation + transposition, the dry calibration pass, the activation-scale update and the fp8 forward
#   eval_fwd:  the fp8 forward alone (scales stay)        bwd1: maxima only (bf16 GEMMs)        bwd2: the gradient-scale update first
#   opt_step:  weight-scale update, the update itself (transposed copy fused), gradient-scale update        bwd3: no scale update
LAUNCHES = {"train_fwd": 470, "eval_fwd": 232, "bwd1": 572, "bwd2": 513, "opt_step": 3, "bwd3": 512}


def _state(core):
    return core._fp8


def _fp8_shadows_consistent(core, opt=None):
    """The transposed shadow is the byte-exact transposition of the shadow, and the shadow dequantises to the fp32 weights within e4m3
    precision (3 mantissa bits: 2^-4 relative; the subnormal step; the scale is one update old), for every shadowed weight."""
    st = _state(core)
    q, qt, w_in = st.q, st.qt, st.w_in.tolist()
    for slot, (off, num) in enumerate(st.weights):
        assert torch.equal(qt[off:off + num].view(w_in[slot], num // w_in[slot]), q[off:off + num].view(num // w_in[slot], w_in[slot]).t()), slot
        w = core.flat_params[off:off + num]
        deq = q[off:off + num].view(torch.float8_e4m3fn).float() / st.weight.scale[slot]
        err = (deq - w).abs() - (0.0625 * w.abs() + 0.002 / float(st.weight.scale[slot]) + 4e-4)
        assert float(err.max()) <= 0, (slot, float(err.max()))


def _counted(lib, counts, phase, fn):
    torch.cuda.synchronize()
    lib.crct_prof_reset()
    res = fn()
    torch.cuda.synchronize()
    counts[phase] = lib.crct_prof_stamp_count()
    return res


def _sequence():
    """The whole sequence, once: what each test below asserts is recorded here as it happens."""
    from crct.optim import get_optimizer
    from test_step_gpu import build_model
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                           v_hidden_dropout_prob=0.0, v_attention_probs_dropout_prob=0.0)
    batch = S.make_batch(3, 31, 7, 2048, seed=103)
    model, params = build_model(cfg, C.default_params(fp8=True), weights=None, seed=11)
    core = model.bert_pretrained
    lib = L.load()
    seen, counts = {}, {}
    lib.crct_prof_enable(2)
    try:
        # training forward under grad: the state is created, calibrated by the dry pass and scaled once
        out = _counted(lib, counts, "train_fwd", lambda: step_forward(model, batch, params))
        st = _state(core)
        act0 = st.act.scale.clone()
        seen["train_fwd"] = dict(calibrated=st.calibrated, scaled=st.scaled, act_moved=bool((act0 != 1.0).any()), act_updates=st.act.updates,
                                 act_positive=float(act0.min()) > 0)

        def evaluate():
            model.eval()
            with torch.no_grad():
                ev = step_forward(model, batch, params, output_nsp_scores=True, evaluation=True)
            model.train()
            return ev
        _counted(lib, counts, "eval_fwd", evaluate)
        seen["eval_fwd"] = dict(act_same_bits=torch.equal(st.act.scale, act0), act_updates=st.act.updates)
        # first backward: collects the gradient maxima, its scales stay 1
        _counted(lib, counts, "bwd1", lambda: out[0].backward())
        seen["bwd1"] = dict(bwd_calibrated=st.bwd_calibrated, grad_scale_ones=bool((st.grad.scale == 1.0).all()),
                            grad_amax_nonzero=bool((st.grad.amax > 0).any()), grad_updates=st.grad.updates)
        # second forward + backward, no optimizer in between: the backward pass refreshes the gradient scales itself
        core.zero_flat_grads()
        out = step_forward(model, batch, params)
        _counted(lib, counts, "bwd2", lambda: out[0].backward())
        seen["bwd2"] = dict(grad_updates=st.grad.updates, grad_scale_all_moved=bool((st.grad.scale != 1.0).all()), fresh=st.g_scales_fresh)
        # one fused AdamW step: weight scales before the update, gradient scales behind it
        opt = get_optimizer(params, model)
        seen["fused"] = st.shadow_for(opt._segs)[1]

        def update():
            opt.step()
            opt.synchronize()
        _counted(lib, counts, "opt_step", update)
        seen["opt_step"] = dict(weight_updates=st.weight.updates, grad_updates=st.grad.updates, fresh=st.g_scales_fresh)
        seen["core"] = core                       # (a forward or backward pass rewrites neither the weights nor their shadows)
        # third forward + backward: the optimizer has refreshed the scales already
        opt.zero_grad()
        out = step_forward(model, batch, params)
        _counted(lib, counts, "bwd3", lambda: out[0].backward())
        seen["bwd3"] = dict(grad_updates=st.grad.updates, fresh=st.g_scales_fresh, finite=bool(torch.isfinite(core.flat_grads).all()))
    finally:
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()
    return seen, counts


@pytest.fixture(scope="module")
def sequence():
    return _sequence()


def test_protocol_flags_scales_and_counters(sequence):
    seen, _ = sequence
    assert seen["train_fwd"] == dict(calibrated=True, scaled=True, act_moved=True, act_updates=1, act_positive=True)
    assert seen["eval_fwd"] == dict(act_same_bits=True, act_updates=1)
    assert seen["bwd1"] == dict(bwd_calibrated=True, grad_scale_ones=True, grad_amax_nonzero=True, grad_updates=0)
    assert seen["bwd2"] == dict(grad_updates=1, grad_scale_all_moved=True, fresh=False)
    assert seen["opt_step"] == dict(weight_updates=1, grad_updates=2, fresh=True)
    assert seen["bwd3"] == dict(grad_updates=2, fresh=False, finite=True)


def test_launch_counts_of_each_phase(sequence):
    _, counts = sequence
    print("fp8 library launches per phase:", counts)
    assert counts == LAUNCHES


def test_shadow_descriptor_keeps_the_transposed_copy_in_the_update(sequence):
    seen, _ = sequence
    assert seen["fused"] is True
    _fp8_shadows_consistent(seen["core"])         # after the one step: qt is the byte-exact transposition of q, for every weight
