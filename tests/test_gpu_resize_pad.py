"""Pad on decode (pjd_batch_set_resize_pad, pjd_batch_set_pad_value) on the GPU (run with -m gpu on an MI355X).  Every expectation is
tests/resize_pad_model.py -- the orientation model to the CONTENT's size, pasted into a canvas of fill -- over the oracle's picture, and
every comparison is byte (bit, for floats) equality; never something this library delivered.  Every batch of the matrix holds all eight
orientations, padded pictures of every kind and an unpadded one, so the launch under test is the mixed one.  The fixtures assert on the
CPU, before anything runs on the device, that no expectation is also what a wrong implementation would deliver, and that the wrong
implementations met are exactly those resize_pad_model.WRONG lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import orientation_model as om
import resize_pad_model as pm
from conftest import golden_bytes, ROOT
from test_gpu_resize import HUFF_ERR, _scanned
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
FILTERS = list(om.FILTERS)
ORIS = list(range(1, 9))
FILL = (114, 7, 201)
REC = 40 + 32                                                # a window record and a canvas record per picture

# (source (w, h, seed) of a synthetic picture without symmetry, (tw, th) of Q -- the content, transposed for orientations 5..8 --, pad
# (left, top, right, bottom) of the delivered canvas)
#   (259, 13) + (5, 3, 6, 4): canvas 270 x 20 (24 x 266 transposed); crosses the 256-column tile, the last lane group is ragged, the
#                             second row tile ragged, canvas rows 270 (or 24 + ...) samples apart: every store alignment occurs
#   (256, 8) + (4, 8, 4, 0):  canvas 264 x 16: rectangle and rows on multiples of four samples, so the vector stores are taken
#   (5, 259) + (1, 0, 3, 1):  canvas 9 x 260;   (1, 1) + (4, 4, 4, 4): one sample in 9 x 9
#   (19, 11) with a pad on exactly one side each, with none (the unpadded picture of the mixed launch), and one column short of the canvas
SHAPES = [((600, 40, 51), (259, 13), (5, 3, 6, 4)), ((600, 40, 51), (256, 8), (4, 8, 4, 0)), ((40, 600, 52), (5, 259), (1, 0, 3, 1)),
          ((16, 12, 54), (1, 1), (4, 4, 4, 4)),
          ((61, 45, 53), (19, 11), (3, 0, 0, 0)), ((61, 45, 53), (19, 11), (0, 2, 0, 0)), ((61, 45, 53), (19, 11), (0, 0, 5, 0)),
          ((61, 45, 53), (19, 11), (0, 0, 0, 6)), ((61, 45, 53), (19, 11), (0, 0, 0, 0)), ((61, 45, 53), (19, 11), (0, 0, 1, 0))]
N_MATRIX_FLOAT = 2                                           # the first two shapes, and the 1 x 1 content, run in all three float types


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _filter(b, filt):
    import pjd_amd
    if filt != "bilinear":
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if filt == "antialias" else pjd_amd.RESIZE_BICUBIC)


def _layout(pic, planar):
    return np.ascontiguousarray(pic.transpose(2, 0, 1)) if planar else pic


def _canvas(tw, th, o, pad):
    """(out_h, out_w) to hand to set_resize: Q's target tw x th as it is delivered, plus the pad."""
    cw, ch = (th, tw) if o >= 5 else (tw, th)
    return (ch + pad[1] + pad[3], cw + pad[0] + pad[2])


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


def _constants():
    from pjd_amd import tensors
    return tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sources(port):
    """{(w, h, seed): (jpeg bytes, the oracle's picture)}"""
    synth = _synth()
    out = {}
    for key in sorted({s for s, _, _ in SHAPES}):
        data = synth.make(key[0], key[1], key[2], 90, synth.SUB_444)
        out[key] = (data, port.decode(data)["rgb"])
    return out


def _case(rgb, win, tw, th, o, pad, filt, met, what):
    """The expectation for the content tw x th (Q's target) in orientation o inside its canvas, checked against the wrong models."""
    out_h, out_w = _canvas(tw, th, o, pad)
    want = pm.padded(rgb, win, out_w, out_h, pad, FILL, o, filt)
    met |= pm.assert_not_a_wrong_model(pm.wrong_models(rgb, win, out_w, out_h, pad, FILL, o, filt), want, what)
    return want


@pytest.fixture(scope="module")
def shape_cases(sources):
    """[(jpeg, (out_h, out_w), o, {filter: expectation}, pad)]: every shape in every orientation, 80 pictures.  Also the place where the set
    of wrong models met by this module's expectations is held against the list."""
    out, met = [], set()
    for src, (tw, th), pad in SHAPES:
        data, rgb = sources[src]
        for o in ORIS:
            out.append((data, _canvas(tw, th, o, pad), o, {f: _case(rgb, None, tw, th, o, pad, f, met, (src, tw, th, o, pad, f)) for f in FILTERS}, pad))
    # ... those of the float tests and of the window with PJD_RW_HFLIP, which the other fixtures meet again
    scale, bias = _constants()
    c = out[0]
    for dtype in DTYPES:
        for value in (None, (0.0, 0.0, 0.0)):
            want = pm.normalized(c[3]["bilinear"], c[1][1], c[1][0], c[4], dtype, scale, bias, value)
            met |= pm.assert_not_a_wrong_model(pm.wrong_models_float(c[3]["bilinear"], c[1][1], c[1][0], c[4], FILL, dtype, scale, bias, value), want, (dtype, value), bits=True)
    _case(sources[(61, 45, 53)][1], HFLIP_WIN, 19, 11, 1, (5, 3, 6, 4), "bilinear", met, "hflip")
    assert met == set(pm.WRONG), met ^ set(pm.WRONG)
    return out


HFLIP_WIN = dict(x=3, y=5, w=40, h=30, flags=1)


def _run(ctx, cases, planar, filt, dtype=0, wins=None, flags=0, value=None, scanned=None):
    """One batch over cases [(jpeg, (out_h, out_w), o, ..., pad)] in the library's own buffer -> (pictures, statuses, info)."""
    scale, bias = _constants()
    sc = scanned or [_scanned(c[0], flags) for c in cases]
    with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
        b.set_resize([c[1] for c in cases])
        b.set_resize_pad([c[4] for c in cases], FILL)
        b.set_orientation([c[2] for c in cases])
        if wins is not None:
            b.set_resize_window(wins)
        _filter(b, filt)
        if dtype:
            b.set_normalize(dtype, scale, bias)
            if value is not None:
                b.set_pad_value(value)
        for i, c in enumerate(cases):
            assert b.output_shape(i) == ((3,) + tuple(c[1]) if planar else tuple(c[1]) + (3,))
            assert b.output_size(i) == 3 * c[1][0] * c[1][1] * (nm.ESIZE[dtype] if dtype else 1)
        b.upload(); b.decode()
        outs, st = b.download()
        return outs, st, b.info()


def _want(c, planar, filt, dtype=0, value=None):
    scale, bias = _constants()
    u8 = c[3][filt]
    return _layout(pm.normalized(u8, c[1][1], c[1][0], c[4], dtype, scale, bias, value) if dtype else u8, planar)


def _check(cases, outs, planar, filt, dtype=0, value=None):
    for k, (c, o) in enumerate(zip(cases, outs)):
        want = _want(c, planar, filt, dtype, value)
        assert o.shape == want.shape, (k, c[1], c[2])
        bad = np.argwhere(nm.bits(o) != nm.bits(want)) if dtype else np.argwhere(o != want)
        assert bad.size == 0, (k, "canvas (h, w)", c[1], "orientation", c[2], "pad", c[4], filt, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 1: every shape in every orientation, one launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_shape_in_every_orientation(ctx, shape_cases, fmt, filt):
    planar = fmt == "planar"
    outs, st, info = _run(ctx, shape_cases, planar, filt)
    assert st == [0] * len(shape_cases)
    assert info["out_bytes"] == sum(3 * h * w for _, (h, w), _, _, _ in shape_cases), "out_bytes is the sum of the canvases"
    _check(shape_cases, outs, planar, filt)


def _float_cases(shape_cases):
    cases = shape_cases[0:8 * N_MATRIX_FLOAT] + shape_cases[24:32]
    assert {c[4] for c in cases} == {(5, 3, 6, 4), (4, 8, 4, 0), (4, 4, 4, 4)} and (9, 9) in {c[1] for c in cases}
    return cases


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_normalized_output_in_every_orientation(ctx, shape_cases, fmt, filt, dtype):
    """The two large shapes and the 1 x 1 content in the library's own buffer (aligned: the vector stores) for every filter, layout
    and dtype: the border is the normalised fill."""
    planar = fmt == "planar"
    cases = _float_cases(shape_cases)
    outs, st, _ = _run(ctx, cases, planar, filt, dtype)
    assert st == [0] * len(cases)
    _check(cases, outs, planar, filt, dtype)


# 3e-6 lies between 2^-25 and 2^-14: a binary16 subnormal, neither zero nor normal; -0.0 keeps its sign
@pytest.mark.parametrize("value", [(0.0, 0.0, 0.0), (3e-6, -3e-6, -0.0)], ids=["zero", "f16_subnormal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_pad_value_replaces_the_normalised_fill(ctx, shape_cases, fmt, dtype, value):
    planar = fmt == "planar"
    cases = _float_cases(shape_cases)
    scale, bias = _constants()
    c = cases[0]
    want = pm.normalized(c[3]["bilinear"], c[1][1], c[1][0], c[4], dtype, scale, bias, value)
    assert pm.assert_not_a_wrong_model(pm.wrong_models_float(c[3]["bilinear"], c[1][1], c[1][0], c[4], FILL, dtype, scale, bias, value), want, value, bits=True)
    m = pm.border_mask(c[1][1], c[1][0], c[4])
    for ch in range(3):                                      # the border bits are the model's conversion of the value, and nothing else
        assert (nm.bits(want[..., ch])[m] == nm.bits(pm.convert(value[ch], dtype))).all()
    if dtype == nm.DT_F16 and value[0]:
        assert 0 < int(nm.bits(pm.convert(value[0], dtype)).reshape(-1)[0]) < 0x0400
    outs, st, _ = _run(ctx, cases, planar, "bilinear", dtype, value=value)
    assert st == [0] * len(cases)
    _check(cases, outs, planar, "bilinear", dtype, value)


# ---- 2: bound, unaligned output with guard bands, decoded twice over different pre-fills -------------------------------------------------------
@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_unaligned_output_over_two_prefills(ctx, shape_cases, fmt, filt, dtype):
    """The first three shapes (floats: the first and as many of the next three as the donor holds) in all orientations bound into the decoded pictures of two donor batches (two different pre-fills of
    caller-owned memory): uint8 canvases 1, 2 and 3 bytes off a dword, float canvases an odd number of elements off, gaps between them
    as guard bands.  After each decode every canvas is the model's, border included, and every byte outside the canvases still the
    donor's."""
    import pjd_amd
    planar = fmt == "planar"
    es = nm.ESIZE[dtype] if dtype else 1
    scale, bias = _constants()
    # what fits the smaller donor (562 500 bytes) at this element size; the 270 x 20 canvases, where every alignment occurs, always (in
    # binary32 without orientation 1, whose store path is that of 2: the seven others are 508 608 bytes with the 9 x 9 canvases)
    cases = {1: shape_cases[0:24], 2: shape_cases[0:8] + shape_cases[16:32], 4: shape_cases[1:8] + shape_cases[24:32]}[es]
    assert {c[4] for c in cases} >= {(5, 3, 6, 4), (4, 4, 4, 4) if es > 1 else (4, 8, 4, 0)} and {c[2] for c in cases} == set(ORIS)
    results = []
    for donor_name in ("big_640x480_420_q85", "big_500x375_444_q92_opt"):
        donor_sc = _scanned(golden_bytes(donor_name), 0)
        with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
            donor.upload(); donor.decode()
            (pattern,), _ = donor.download()
            pattern = pattern.reshape(-1).copy()
            mem, cap = donor.device_output(0), donor.output_size(0)
            assert mem % 256 == 0
            sc = [_scanned(c[0], 0) for c in cases]
            with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
                b.set_resize([c[1] for c in cases])
                b.set_resize_pad([c[4] for c in cases], FILL)
                b.set_orientation([c[2] for c in cases])
                _filter(b, filt)
                if dtype:
                    b.set_normalize(dtype, scale, bias)
                offs, pos = [], 7 * es
                for i in range(b.n):
                    while (pos // es) % 4 != (i % 3) + 1:      # 1, 2, 3 elements past a multiple of four elements; the gap is a guard band
                        pos += es
                    offs.append(pos)
                    pos += b.output_size(i) + 5 * es
                assert pos <= cap and sorted({(o // es) % 4 for o in offs}) == [1, 2, 3]
                b.bind_output(mem, cap, offs)
                b.upload(); b.decode()
                outs, st = b.download()
                sizes = [b.output_size(i) for i in range(b.n)]
            (after,), _ = donor.download()
            after = after.reshape(-1)
        assert st == [0] * len(cases)
        _check(cases, outs, planar, filt, dtype)
        covered = np.zeros(cap, bool)
        for c, off, size in zip(cases, offs, sizes):
            want = _want(c, planar, filt, dtype)
            assert size == want.nbytes and after[off:off + size].tobytes() == want.tobytes(), (c[1], c[2])
            covered[off:off + size] = True
        stray = np.flatnonzero(~covered & (after != pattern))
        assert stray.size == 0, f"bytes outside every canvas were written, first at {stray[:8]}"
        results.append(pattern[:offs[-1] + sizes[-1]])
    assert not np.array_equal(results[0], results[1]), "the two pre-fills differ"


# ---- 2b: everything at once ---------------------------------------------------------------------------------------------------------------------
# (Q's target, orientation, pad, window): a content 259 columns wide (a second, ragged column tile) that takes no window, a transposed
# one under a mirrored window, a picture without a pad under a half turn and a window with offsets, a content of 9 rows (a second,
# ragged row tile) mirrored
STACKED = [((259, 5), 1, (5, 3, 6, 4), None), ((20, 9), 6, (1, 0, 3, 1), dict(x=3, y=5, w=40, h=30, flags=1)),
           ((19, 11), 3, (0, 0, 0, 0), dict(x=1, y=2, w=50, h=40, vw=25, vh=14, ox=4, oy=2)), ((7, 9), 2, (0, 2, 0, 0), None)]


@pytest.mark.parametrize("fmt,filt", [("rgb8", "antialias"), ("planar", "bicubic")])
def test_every_setter_stacked_in_one_bound_batch(ctx, sources, fmt, filt):
    """One batch that every setter has touched: a pad with one picture that has none, orientations 1, 2, 3 and the transposing 6,
    windows of which two are all zero and one is mirrored, a table-driven filter, binary16 output with a pad value, bound into
    caller-owned memory at offsets of the caller's choosing.  Bit for bit the models', and not a byte outside the canvases."""
    import pjd_amd
    planar, dtype, value = fmt == "planar", nm.DT_F16, (0.5, -1.0, 3e-6)
    scale, bias = _constants()
    data, rgb = sources[(61, 45, 53)]
    met = set()
    cases = [(data, _canvas(tw, th, o, pad), o, {filt: _case(rgb, win, tw, th, o, pad, filt, met, (tw, th, o, pad))}, pad) for (tw, th), o, pad, win in STACKED]
    assert cases[0][1] == (12, 270) and cases[1][1] == (21, 13) and {c[2] for c in cases} == {1, 2, 3, 6}
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        donor.upload(); donor.decode()
        (pattern,), _ = donor.download()
        pattern = pattern.reshape(-1).copy()
        mem, cap = donor.device_output(0), donor.output_size(0)
        sc = [_scanned(c[0], 0) for c in cases]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize([c[1] for c in cases])
            b.set_resize_pad([c[4] for c in cases], FILL)
            b.set_orientation([c[2] for c in cases])
            b.set_resize_window([s[3] for s in STACKED])
            _filter(b, filt)
            b.set_normalize(dtype, scale, bias)
            b.set_pad_value(value)
            offs, pos = [], 6
            for i in range(b.n):                                 # every canvas one element past a dword, the gaps are guard bands
                while pos % 4 != 2:
                    pos += 2
                offs.append(pos)
                pos += b.output_size(i) + 6
            assert pos <= cap
            b.bind_output(mem, cap, offs)
            b.upload(); b.decode()
            outs, st = b.download()
            sizes = [b.output_size(i) for i in range(b.n)]
        (after,), _ = donor.download()
        after = after.reshape(-1)
    assert st == [0] * len(cases)
    _check(cases, outs, planar, filt, dtype, value)
    covered = np.zeros(cap, bool)
    for c, off, size in zip(cases, offs, sizes):
        want = _want(c, planar, filt, dtype, value)
        assert size == want.nbytes and after[off:off + size].tobytes() == want.tobytes(), (c[1], c[2])
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every canvas were written, first at {stray[:8]}"


# ---- 3: the other paths into the launch -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_pictures(port):
    out = {}
    for n in ("noise_80x96_422_q50_opt", HUFF_ERR[0]):
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    assert out[HUFF_ERR[0]][0] != 0
    return out


@pytest.mark.parametrize("mode", ["scale_1_2", "entropy_error", "sequential", "libjpeg", "window_hflip", "graph"])
@pytest.mark.parametrize("filt", FILTERS)
def test_other_paths_into_the_launch(ctx, fixture_pictures, filt, mode):
    """PJD_F_SCALE_1_2 in front, a fixture with an entropy-coding error (its status kept, grey in the content, fill in the border), the
    exact kernel (PJD_F_FORCE_SEQUENTIAL), a PJD_F_LIBJPEG picture, a window with PJD_RW_HFLIP (which mirrors the content, not the
    rectangle), and a captured graph replayed twice: all eight orientations, planar, the content 19 x 11 with the pad (5, 3, 6, 4)."""
    import pjd_amd
    pad, win, scanned, jpeg = (5, 3, 6, 4), None, None, None
    if mode == "libjpeg":
        from test_gpu_libjpeg import BIG, scanned as lj_scanned
        scanned = [lj_scanned(BIG)[0] for _ in ORIS]
        status, src = 0, lj_scanned(BIG)[1]                  # the fixture's picture is libjpeg's own decode
    else:
        name = HUFF_ERR[0] if mode == "entropy_error" else "noise_80x96_422_q50_opt"
        status, rgb = fixture_pictures[name]
        jpeg = golden_bytes(name)
        src = box(rgb, 2 if mode == "scale_1_2" else 1)
    flags = 16 if mode == "scale_1_2" else pjd_amd.F_FORCE_SEQUENTIAL if mode == "sequential" else 0
    if mode == "window_hflip":
        win = dict(x=3, y=5, w=40, h=30, flags=pjd_amd.RW_HFLIP)
    met = set()
    cases = [(jpeg, _canvas(19, 11, o, pad), o, {filt: _case(src, win, 19, 11, o, pad, filt, met, (mode, o))}, pad) for o in ORIS]
    if mode == "window_hflip":
        assert "rectangle_mirrored_by_hflip" in met
    if mode != "graph":
        outs, st, info = _run(ctx, cases, True, filt, flags=flags, wins=[win] * len(cases) if win else None, scanned=scanned)
        if mode == "sequential":
            assert info["n_sequential"] == len(cases)
    else:
        sc = [_scanned(c[0], 0) for c in cases]
        with ctx.batch([x.desc for x in sc], _fmt(True)) as b:
            b.set_resize([c[1] for c in cases])
            b.set_resize_pad([c[4] for c in cases], FILL)
            b.set_orientation([c[2] for c in cases])
            _filter(b, filt)
            b.upload(); b.capture()
            for _ in range(2):
                b.decode(); b.sync()
            outs, st = b.download()
    assert list(st) == [status] * len(cases)
    _check(cases, outs, True, filt)


# ---- 4: the identity, the records, the launches' names ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_all_zero_records_equal_a_batch_without_the_call(ctx, fmt, filt):
    import pjd_amd
    names = ["big_640x480_420_q85", "env_61x45_444_q85_opt", "gray_33x70", HUFF_ERR[0]]
    sizes = [(224, 224), (9, 257), (70, 33), (12, 11)]
    res = []
    for call in (False, True):
        sc = [_scanned(golden_bytes(n), 0) for n in names]
        with ctx.batch([x.desc for x in sc], _fmt(fmt == "planar")) as b:
            b.set_resize(sizes)
            if call:
                b.set_resize_pad([None, (0, 0, 0, 0), dict(), pjd_amd.ResizePad()], FILL)
            b.set_orientation([1, 6, 1, 3])
            b.set_resize_window([None, dict(x=1, y=2, w=50, h=40, flags=1), None, None])
            _filter(b, filt)
            b.upload()
            per, _ = b.decode_timed()
            outs, st = b.download()
            info = b.info()
            res.append((outs, st, [b.output_size(i) for i in range(b.n)], info["out_bytes"], info["device_bytes"], list(per)))
    assert res[0][1:] == res[1][1:] and any(res[0][1]) and "pad" not in res[1][5] and res[1][5][-1] == "resize"
    for n, a, c in zip(names, res[0][0], res[1][0]):
        assert a.shape == c.shape and np.array_equal(a, c), n


def test_the_records_are_counted_once_and_the_launch_is_named_pad(ctx, sources):
    import pjd_amd
    data, _ = sources[(61, 45, 53)]
    n = len(ORIS)
    sc = [_scanned(data, 0) for _ in ORIS]
    pads = [(5, 3, 6, 4)] * (n - 1) + [None]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize([_canvas(30, 20, o, p or (0, 0, 0, 0)) for o, p in zip(ORIS, pads)])
        before = b.info()
        b.set_resize_pad(pads, FILL)
        assert b.info()["device_bytes"] == before["device_bytes"] + REC * n + 4 * (n + 1), "the records and the prefix sum are counted"
        b.set_orientation(ORIS)
        b.set_resize_window([dict(x=1, y=1, w=50, h=40)] * n)
        assert b.info()["device_bytes"] == before["device_bytes"] + REC * n + 4 * (n + 1), "... and orientation and windows take none of their own"
        assert b.info()["out_bytes"] == before["out_bytes"] == sum(b.output_size(i) for i in range(n)), "out_bytes stays the sum of the canvases"
        b.upload()
        per, total = b.decode_timed()
        assert list(per)[-2:] == ["resize", "pad"] and per["pad"] > 0 and per["resize"] > 0, per
        assert total >= per["resize"] + per["pad"]


def test_the_longest_chain_of_a_padded_batch_fits_the_timings(ctx, sources):
    """A flagged picture, one forced to the exact kernel and a plain one, resized and padded: every launch the decode can name."""
    import pjd_amd
    from test_gpu_libjpeg import BIG, scanned as lj_scanned
    data, _ = sources[(61, 45, 53)]
    sc = [lj_scanned(BIG)[0], lj_scanned(BIG, pjd_amd.F_FORCE_SEQUENTIAL)[0], _scanned(data, pjd_amd.F_FORCE_SEQUENTIAL), _scanned(data, 0)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(20, 30)] * 4)
        b.set_resize_pad([(5, 3, 6, 4)] * 4, FILL)
        b.upload()
        per, _ = b.decode_timed()
    assert {"idct_std", "exact_path", "colour_std", "resize", "pad"} <= set(per), per
    assert len(per) + 1 < pjd_amd.MAX_KERNELS, per                                      # none was cut off at PJD_MAX_KERNELS


# ---- 5: call order and arguments ----------------------------------------------------------------------------------------------------------------
def _pads(*recs):
    import pjd_amd
    return (pjd_amd.ResizePad * len(recs))(*[pjd_amd.ResizePad(*r) for r in recs])


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_set_resize_pad_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok, zero, fill = _pads((1, 2, 3, 4), (0, 0, 5, 0)), _pads((0, 0, 0, 0), (0, 0, 0, 0)), (C.c_uint8 * 3)(*FILL)
    one = _f3(1.0, 1.0, 1.0)
    win = (pjd_amd.ResizeWindow * 2)()
    assert L.pjd_batch_set_resize_pad(None, ok, fill) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # no resize is set
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == 0
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # twice
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_pad(b._h, zero, fill) == 0
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # twice, the first one all zero
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.set_orientation([1, 1])
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after set_orientation
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_window(b._h, win) == 0
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after set_resize_window
    for filt in (pjd_amd.RESIZE_BILINEAR, pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BICUBIC):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_resize_filter(filt)
            assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE               # after set_resize_filter
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0          # which sets the identity resize itself
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after upload
        b.decode()
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after decode
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload(); b.capture()
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # after capture
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE               # after bind_output
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == E_STATE                   # a BMP batch takes no resize, so no pad
    for bad in (dict(pads=[None]), dict(pads=[None, None], fill=(0, 0)), dict(pads=[None, None], fill=(0, 0, 256))):
        with pytest.raises(ValueError):
            with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
                b.set_resize(sizes)
                b.set_resize_pad(**bad)


def test_set_pad_value_state_and_argument_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok, zero, fill = _pads((1, 2, 3, 4), (0, 0, 5, 0)), _pads((0, 0, 0, 0), (0, 0, 0, 0)), (C.c_uint8 * 3)(*FILL)
    one, val = _f3(1.0, 1.0, 1.0), _f3(0.0, 0.5, -1.0)
    assert L.pjd_batch_set_pad_value(None, val) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_pad_value(b._h, val) == E_STATE                         # the batch has no pad
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == 0
        assert L.pjd_batch_set_pad_value(b._h, val) == E_STATE                         # before set_normalize
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_BF16, one, one) == 0
        assert L.pjd_batch_set_pad_value(b._h, None) == E_ARG                          # a null array, and values that are not finite,
        for bad in (float("nan"), float("inf"), -float("inf")):                      # change nothing: the call is still open
            assert L.pjd_batch_set_pad_value(b._h, _f3(0.0, bad, 0.0)) == E_ARG, bad
        assert L.pjd_batch_set_pad_value(b._h, val) == 0
        assert L.pjd_batch_set_pad_value(b._h, val) == E_STATE                         # twice
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_pad(b._h, zero, fill) == 0
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0
        assert L.pjd_batch_set_pad_value(b._h, val) == 0                               # a pad of all-zero records is a pad: the value has no border to fill
    for step in ("upload", "capture", "decode"):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == 0
            assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
            b.upload()
            if step == "capture":
                b.capture()
            if step == "decode":
                b.decode()
            assert L.pjd_batch_set_pad_value(b._h, val) == E_STATE, step
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            assert L.pjd_batch_set_resize_pad(b._h, ok, fill) == 0
            assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_pad_value(b._h, val) == E_STATE                     # after bind_output


def test_set_resize_pad_argument_errors_name_the_picture_and_leave_the_batch_as_it_was(ctx, port):
    import pjd_amd
    import resize_model
    L = pjd_amd.dev_lib()
    names = ["gray_33x70", "env_61x45_420_q100_opt"]
    rgb = [port.decode(golden_bytes(n))["rgb"] for n in names]
    sc = [_scanned(golden_bytes(n), 0) for n in names]
    sizes = [(31, 17), (20, 30)]
    fill = (C.c_uint8 * 3)(*FILL)
    M = 2 ** 32 - 1
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_resize_pad(b._h, None, fill) == E_ARG                   # a null array, a null fill: nothing changes
        assert L.pjd_batch_set_resize_pad(b._h, _pads((1, 1, 1, 1), (1, 1, 1, 1)), None) == E_ARG
        for bad in ((15, 0, 15, 0), (30, 0, 0, 0), (0, 10, 0, 10), (0, 0, 0, 20), (M, 0, 2, 0), (0, 2 ** 31, 0, 2 ** 31)):
            assert L.pjd_batch_set_resize_pad(b._h, _pads((1, 2, 3, 4), bad), fill) == E_ARG, bad
            assert b"picture 1" in L.pjd_last_error(ctx._h), (bad, L.pjd_last_error(ctx._h))
        assert L.pjd_batch_set_resize_pad(b._h, _pads((9, 0, 8, 0), (1, 2, 3, 4)), fill) == E_ARG      # 17 columns: 9 + 8 leaves none
        assert b"picture 0" in L.pjd_last_error(ctx._h)
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                         # after the refused calls: unpadded
        outs, st = b.download()
    assert st == [0, 0]
    for p, (th, tw), o in zip(rgb, sizes, outs):
        assert np.array_equal(o, resize_model.resize(p, tw, th))
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:                       # ... and the call is still open after a refusal
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_pad(b._h, _pads((9, 0, 8, 0), (0, 0, 0, 0)), fill) == E_ARG
        b.set_resize_pad([(8, 0, 8, 0), (1, 2, 3, 4)], FILL)                           # a content of exactly one column
        b.set_orientation([8, 3])
        b.upload(); b.decode()
        outs, st = b.download()
    for p, (th, tw), o, ori, pad in zip(rgb, sizes, outs, (8, 3), ((8, 0, 8, 0), (1, 2, 3, 4))):
        assert np.array_equal(o, pm.padded(p, None, tw, th, pad, FILL, ori)), ori


# ---- 6: the torch side, in a child process (tests/resize_pad_torch_cases.py imports torch first) ----------------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "resize_pad_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_tensor_helpers_with_letterbox():
    """letterbox="center" uint8 and letterbox="topleft" with pad_value=0, bf16, channels_last against the model, and both within one
    level of torch's interpolate followed by pad for the bilinear and bicubic filters."""
    _torch_case("letterbox")
