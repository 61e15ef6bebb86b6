"""The order of the batch setters (include/pjd.h) on the GPU (run with -m gpu on an MI355X): which call is refused after which, with
which return code and which pjd_last_error text, and which message wins where several apply.

The expectation is the model below, written from the header's "Once, after ... and before ..." sentences and nothing of the library:

    the stages, in the order a batch passes them    views < resize < pad < orientation < window < filter < normalize < pad_value
                                                    < bind_output < upload
    a call is refused (PJD_E_STATE), first reason that applies:
      1. a stage it needs has not been passed       "<call>: no resize is set ..." / "... has no pad ..." / "... is not normalised ..."
      2. it was made before and may not be repeated "<call>: already set for this batch"        (bind_output and upload may)
      3. a later stage has been passed              "<call> after <the earliest such stage>"
    set_normalize on a batch without a resize sets the identity resample: the resize stage is passed with it
    the one exception: set_views names set_normalize, not set_resize, where the batch is normalised
    bind_output and upload (and decode, capture) refuse a batch that has views and no resample, behind everything above

One baseline 4:2:0 picture of 16 x 16, PJD_OUT_RGB8, a fresh batch per case, every argument valid and as small as it goes: a refused
call is refused for its place in the order alone.  bind_output gets the (never uploaded) result buffer of a second batch."""
import os
import re
import sys

import numpy as np
import pytest

import normalize_model as nm
import resize_pad_model as pm
from conftest import ROOT

pytestmark = pytest.mark.gpu

OK, E_STATE = 0, -5

# ---- the model ---------------------------------------------------------------------------------------------------------------------------
CALLS = ("set_views", "set_resize", "set_resize_pad", "set_orientation", "set_resize_window", "set_resize_filter", "set_normalize",
         "set_pad_value", "bind_output", "upload")
NEEDS = {"set_resize_pad": ("set_resize",), "set_orientation": ("set_resize",), "set_resize_window": ("set_resize",),
         "set_resize_filter": ("set_resize",), "set_pad_value": ("set_resize_pad", "set_normalize")}
MISSING = {"set_resize": "no resize is set (pjd_batch_set_resize first)",
           "set_resize_pad": "the batch has no pad (pjd_batch_set_resize_pad first)",
           "set_normalize": "the batch is not normalised (pjd_batch_set_normalize first)"}
REPEATABLE = ("bind_output", "upload")
NO_RESAMPLE = "%s: the batch has views but no resample (pjd_batch_set_resize or pjd_batch_set_normalize first)"


class Model:
    """The stages a batch has passed, and what the next call answers: (code, text), text None for PJD_OK."""

    def __init__(self):
        self.passed = set()

    def call(self, name):
        p = self.passed
        for need in NEEDS.get(name, ()):
            if need not in p:
                return E_STATE, f"{name}: {MISSING[need]}"
        if name in p and name not in REPEATABLE:
            return E_STATE, f"{name}: already set for this batch"
        later = [c for c in CALLS[CALLS.index(name) + 1:] if c in p]
        if later:
            behind = "set_normalize" if name == "set_views" and "set_normalize" in p else later[0]
            return E_STATE, f"{name} after {behind}"
        if name in REPEATABLE and "set_views" in p and "set_resize" not in p:
            return E_STATE, NO_RESAMPLE % name
        p.add(name)
        if name == "set_normalize":
            p.add("set_resize")
        return OK, None


def needed(names):
    """Every stage the calls `names` need, and what those need."""
    out = set()
    todo = list(names)
    while todo:
        for r in NEEDS.get(todo.pop(), ()):
            if r not in out:
                out.add(r)
                todo.append(r)
    return out


# ---- the batch ---------------------------------------------------------------------------------------------------------------------------
FILL, PAD_VALUE = (7, 8, 9), (0.5, -0.25, 2.0)
SCALE, BIAS = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
NO_PAD = (0, 0, 0, 0)


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """(the bytes, the scanned picture) of the 16 x 16 picture every case decodes"""
    import pjd_amd
    synth = _synth()
    data = synth.make(16, 16, 41, 85, synth.SUB_420, 0)
    s = pjd_amd.Scanned(data)
    assert s.valid
    return data, s


@pytest.fixture(scope="module")
def memory(ctx):
    """(address, bytes) of device memory for bind_output: the result buffer of a batch of one 64 x 64 picture, never uploaded"""
    import pjd_amd
    synth = _synth()
    s = pjd_amd.Scanned(synth.make(64, 64, 42, 85, synth.SUB_420, 0))
    assert s.valid
    donor = ctx.batch([s.desc], pjd_amd.OUT_RGB8)
    assert donor.device_output(0) and donor.packed_size() >= 64 * 64 * 3
    yield donor.device_output(0), donor.packed_size()
    donor.destroy()


def _apply(b, name, memory):
    import pjd_amd
    n = b.n_out
    if name == "set_views":
        b.set_views([0, 0])
    elif name == "set_resize":
        b.set_resize([(8, 8)] * n)
    elif name == "set_resize_pad":
        b.set_resize_pad([None] * n, FILL)                  # the all-zero record: the canvas is the target
    elif name == "set_orientation":
        b.set_orientation([1] * n)
    elif name == "set_resize_window":
        b.set_resize_window([None] * n)                     # the whole picture
    elif name == "set_resize_filter":
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
    elif name == "set_normalize":
        b.set_normalize(nm.DT_F32, SCALE, BIAS)
    elif name == "set_pad_value":
        b.set_pad_value(PAD_VALUE)
    elif name == "bind_output":
        b.bind_output(*memory)
    else:
        getattr(b, name)()                                  # upload, decode, capture, decode_timed


def _error(ctx):
    return ctx.L.pjd_last_error(ctx._h).decode()


def _call(ctx, b, name, memory):
    """The call on the batch: (code, text), text None for PJD_OK -- which must leave the context's error text as it was."""
    import pjd_amd
    before = _error(ctx)
    try:
        _apply(b, name, memory)
    except pjd_amd.PjdError as e:
        return int(re.search(r"failed \((-?\d+)\)", str(e)).group(1)), _error(ctx)
    assert _error(ctx) == before, (name, before, _error(ctx))
    return OK, None


def _step(ctx, b, model, name, memory, log):
    got, want = _call(ctx, b, name, memory), model.call(name)
    log.append((name, got))
    assert got == want, (log, want)
    return got


# ---- every ordered pair of the ten calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", CALLS)
@pytest.mark.parametrize("first", CALLS)
def test_pair(ctx, small, memory, first, second):
    """What `first` and `second` need (themselves apart) in canonical order, then `first`, then `second`: every answer is the model's
    (a needed call may itself be refused: set_resize_pad where set_resize is the second call of the pair)."""
    import pjd_amd
    model, log = Model(), []
    with ctx.batch([small[1].desc], pjd_amd.OUT_RGB8) as b:
        for name in CALLS:
            if name in needed((first, second)) and name not in (first, second):
                _step(ctx, b, model, name, memory, log)
        _step(ctx, b, model, first, memory, log)
        _step(ctx, b, model, second, memory, log)


# ---- full house: everything else set, which message wins ------------------------------------------------------------------------------------
FULL_HOUSE = {"set_views": "set_views after set_normalize",                  # not "after set_resize": the exception
              "set_resize": "set_resize: already set for this batch",        # set_normalize brought the resize
              "set_resize_pad": "set_resize_pad after set_orientation",
              "set_orientation": "set_orientation after set_resize_window",
              "set_resize_window": "set_resize_window after set_resize_filter",
              "set_resize_filter": "set_resize_filter after set_normalize",
              "set_normalize": "set_normalize after bind_output",
              "set_pad_value": "set_pad_value after bind_output",
              "bind_output": "bind_output after upload",
              "upload": None}


@pytest.mark.parametrize("last", CALLS)
def test_full_house(ctx, small, memory, last):
    """Every other call in canonical order (but those that need `last`), then `last`: the one message the precedence picks, here
    spelled out as well as asked of the model."""
    import pjd_amd
    model, log = Model(), []
    with ctx.batch([small[1].desc], pjd_amd.OUT_RGB8) as b:
        for name in CALLS:
            if name != last and last not in needed((name,)):
                assert _step(ctx, b, model, name, memory, log) == (OK, None)
        got = _step(ctx, b, model, last, memory, log)
    assert got == ((E_STATE, FULL_HOUSE[last]) if FULL_HOUSE[last] else (OK, None)), log


def test_pad_value_on_a_bound_batch_without_a_pad_reports_the_pad(ctx, small, memory):
    import pjd_amd
    model, log = Model(), []
    with ctx.batch([small[1].desc], pjd_amd.OUT_RGB8) as b:
        for name in ("set_resize", "set_normalize", "bind_output"):
            assert _step(ctx, b, model, name, memory, log) == (OK, None)
        assert _step(ctx, b, model, "set_pad_value", memory, log) == (E_STATE, "set_pad_value: the batch has no pad (pjd_batch_set_resize_pad first)")


# ---- views without a resample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prefix", [("bind_output", "bind_output"), ("upload", "upload"), ("decode", "decode"), ("capture", "capture"),
                                         ("decode_timed", "decode")])        # the timed decode speaks as the decode
def test_views_without_a_resample(ctx, small, memory, name, prefix):
    import pjd_amd
    with ctx.batch([small[1].desc], pjd_amd.OUT_RGB8) as b:
        assert _call(ctx, b, "set_views", memory) == (OK, None)
        assert _call(ctx, b, name, memory) == (E_STATE, NO_RESAMPLE % prefix)


# ---- a batch that went through all of it works ------------------------------------------------------------------------------------------------
def test_survivor(ctx, port, small, memory):
    """The whole canonical sequence, then upload and two decodes: both views, both times, are the model's bits."""
    import pjd_amd
    rgb = port.decode(small[0])["rgb"]
    assert rgb.shape == (16, 16, 3)
    canvas = pm.padded(rgb, None, 8, 8, NO_PAD, FILL, 1, "antialias")
    want = pm.normalized(canvas, 8, 8, NO_PAD, nm.DT_F32, SCALE, BIAS, PAD_VALUE)
    model, log = Model(), []
    with ctx.batch([small[1].desc], pjd_amd.OUT_RGB8) as b:
        for name in CALLS:
            assert _step(ctx, b, model, name, memory, log) == (OK, None)
        for turn in range(2):
            b.decode()
            outs, st = b.download()
            assert st == [0] and len(outs) == 2
            for v, o in enumerate(outs):
                assert o.shape == want.shape and o.dtype == want.dtype and np.array_equal(nm.bits(o), nm.bits(want)), (turn, v)
