"""Poisoned operands: which output elements of a launch a non-finite input element reaches ("Non-finite values").

A launch is run twice, clean and with one or two poisoned input elements.  The project's fp64 restatement of the launch, run on
the poisoned inputs on the CPU, names the footprint F: the output elements that are non-finite there.  The kernel must then obey

  R1 (arrival)      every element of F is non-finite in the kernel's poisoned output.  NaN against inf is not compared: fp32 may meet
                    inf - inf at another partial sum than fp64 does;
  R2 (containment)  every element outside F carries the BITS of the clean launch (outputs accumulated with float atomics: finite and
                    within a stated absolute budget of the clean launch instead);
  R3                F is neither empty nor everything for at least one output of the case -- a reference that stopped propagating, or
                    one that poisons all it touches, says nothing about where the value went.

There is no tolerance in R1 / R2: the check is about the dependency structure of the kernel (which rows, tiles, heads, batch elements
and stale buffers an output reads), so a wrong index shows as a leaked or a missing element, named in the message.

Outputs are passed as one tensor, or as a dict / list / tuple of tensors (with F of the same structure); None entries are skipped.
"""
import torch

NAN = float("nan")
INF = float("inf")
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def plant(t, index, value):
    """A copy of t with t[index] = value (index: an int, a tuple of ints / slices, as for t[...]).  t itself stays clean."""
    out = t.clone()
    out[index] = value
    return out


def as_float(t):
    """t as fp64 on its device; uint8 tensors are NOT decoded (pass fp8 bytes through .view(torch.float8_...) first)."""
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        return t.to(torch.float32).double()
    return t.double()


def nonfinite(t):
    """bool mask of the NaN / +-inf elements of t (any float type, the fp8 types included)."""
    return ~torch.isfinite(as_float(t))


def bits(t):
    """t's storage reinterpreted as integers of the element size: equality of these is equality of the bits (-0 != +0, NaN == NaN)."""
    t = t.contiguous()
    return t.view(_BITS[t.element_size()])


def _items(x):
    """[(name, tensor)] of a tensor / dict / sequence of tensors, None entries left out."""
    if torch.is_tensor(x):
        return [("", x)]
    if isinstance(x, dict):
        return [(str(k), v) for k, v in x.items() if v is not None]
    return [(str(i), v) for i, v in enumerate(x) if v is not None]


def _like(x, vals):
    if torch.is_tensor(x):
        return vals[0]
    if isinstance(x, dict):
        return dict(zip([k for k, v in x.items() if v is not None], vals))
    return tuple(vals)


def footprint(ref_fn, clean_inputs, poisoned_inputs):
    """F per output of ref_fn: the elements that are non-finite in ref_fn(*poisoned_inputs).  ref_fn(*clean_inputs) must be finite
    everywhere, so that F is the poison's doing.  ref_fn returns a tensor or a dict / sequence of tensors; F has the same structure
    (bool tensors on the CPU)."""
    clean = ref_fn(*clean_inputs)
    for name, t in _items(clean):
        bad = nonfinite(t)
        assert not bool(bad.any()), "reference output %r is non-finite on the CLEAN inputs (%d elements)" % (name, int(bad.sum()))
    out = ref_fn(*poisoned_inputs)
    return _like(out, [nonfinite(t).cpu() for _, t in _items(out)])


def _first(mask):
    return tuple(int(v) for v in mask.nonzero()[0])


def assert_footprint(got_clean, got_poisoned, F, what, atomic=False):
    """R1, R2 and R3 for the outputs of one case.  atomic: False, or the absolute budget (a float, or a dict / sequence of floats per
    output) within which an output accumulated with float atomics must stay equal to the clean launch outside F."""
    if atomic is True:
        raise ValueError("atomic=True says nothing: pass the absolute budget of the atomically accumulated outputs")
    gc, gp, fs = _items(got_clean), _items(got_poisoned), _items(F)
    assert [n for n, _ in gc] == [n for n, _ in gp] == [n for n, _ in fs], (what, [n for n, _ in gc], [n for n, _ in gp], [n for n, _ in fs])
    budgets = [b for _, b in _items(atomic)] if isinstance(atomic, (dict, list, tuple)) else [atomic] * len(fs)
    assert len(budgets) == len(fs), (what, len(budgets), len(fs))
    proper = 0
    for (name, c), (_, p), (_, f), budget in zip(gc, gp, fs, budgets):
        tag = "%s%s" % (what, (" [%s]" % name) if name else "")
        assert tuple(c.shape) == tuple(p.shape) == tuple(f.shape), (tag, tuple(c.shape), tuple(p.shape), tuple(f.shape))
        f = f.to(p.device)
        n = int(f.sum())
        proper += int(0 < n < f.numel())
        bad_clean = nonfinite(c)
        assert not bool(bad_clean.any()), "%s: the CLEAN launch is non-finite at %s" % (tag, _first(bad_clean))
        missing = f & ~nonfinite(p)                       # R1
        if bool(missing.any()):
            i = _first(missing)
            raise AssertionError("%s: R1 (arrival): %d of the %d elements the reference poisons are finite, first at %s (got %r)"
                                 % (tag, int(missing.sum()), n, i, float(as_float(p)[i])))
        if budget:                                        # R2, atomically accumulated output
            d = (as_float(p) - as_float(c)).abs()
            leaked = ~f & ~(d <= float(budget))           # a NaN outside F compares false: leaked
        else:                                             # R2
            leaked = ~f & (bits(p) != bits(c)).view(f.shape)
        if bool(leaked.any()):
            i = _first(leaked)
            raise AssertionError("%s: R2 (containment): %d elements outside the reference's footprint (%d of %d) differ from the clean "
                                 "launch, first at %s (clean %r, poisoned %r)"
                                 % (tag, int(leaked.sum()), n, f.numel(), i, float(as_float(c)[i]), float(as_float(p)[i])))
    if not proper:                                        # R3
        raise AssertionError("%s: R3: no output has a footprint that is neither empty nor everything (sizes %s)"
                             % (what, ["%d of %d" % (int(f.sum()), f.numel()) for _, f in fs]))
