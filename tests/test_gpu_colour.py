"""Colour map on decode (pjd_batch_set_colour) on the GPU (run with -m gpu on an MI355X).  The expectation of every case is
tests/colour_model.py -- Python integers over the text of include/pjd.h -- applied to what the SAME batch delivers as uint8 WITHOUT
set_colour, downloaded once per request; normalised cases put tests/normalize_model.py on top.  Every comparison is byte (bit, for
floats) equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_model as M
import normalize_model as nm
from conftest import golden_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
FIXTURES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61", "err_truncated_eoi_420"]
DTYPES = [0, nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
WIDTHS, HEIGHTS = (1, 3, 5, 37, 259), (1, 7, 9, 33)
FILL = (114, 7, 201)
IDENT = M.IDENTITY
BGR = M.permutation((2, 1, 0))
GRAY = (0.299, 0.587, 0.114, 0.0) * 3
ALL_HIGH = (16.0, 16.0, 16.0, 4096.0) * 3                    # clamps to 255 everywhere
ALL_LOW = (-16.0, -16.0, -16.0, 0.0) * 3                     # clamps to 0 everywhere


def matrices():
    """the eight matrices of the suite: identity, bgr, grey, both saturating ones, three seeded jitters"""
    rng = np.random.default_rng(4242)
    return [IDENT, BGR, GRAY, ALL_HIGH, ALL_LOW] + [M.jitter(rng) for _ in range(3)]


def sizes_for(n):
    """n targets (tw, th) that walk through every width and every height of the suite"""
    return [(WIDTHS[k % len(WIDTHS)], HEIGHTS[(k + k // len(WIDTHS)) % len(HEIGHTS)]) for k in range(n)]


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _scanned(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _chw(a, planar):
    return a if planar else a.transpose(2, 0, 1)


def _layout(chw, planar):
    return chw if planar else np.ascontiguousarray(chw.transpose(1, 2, 0))


def _norm():
    from pjd_amd import tensors
    return tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


def run(ctx, datas, planar, sizes, shape=None, colours=None, views=None, flags=None, dtype=0, graph=False, pad_value=None):
    """One batch in the library's own buffer -> (outputs, statuses, info).  shape(b): the setter calls between set_resize and set_colour."""
    flags = flags or [0] * len(datas)
    sc = [_scanned(d, f) for d, f in zip(datas, flags)]
    with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
        if views is not None:
            b.set_views(views)
        b.set_resize([(th, tw) for tw, th in sizes])
        if shape is not None:
            shape(b)
        if colours is not None:
            b.set_colour(colours)
        if dtype:
            b.set_normalize(dtype, *_norm())
            if pad_value is not None:
                b.set_pad_value(pad_value)
        b.upload()
        if graph:
            b.capture()
            for _ in range(2):
                b.decode(); b.sync()
        else:
            b.decode()
        outs, st = b.download()
        return outs, st, b.info()


def want(base, m, planar, dtype=0, border=None):
    """the model's output for one uncoloured uint8 output `base`: the map, then the normalisation table per channel.  border: None, or
    (left, top, right, bottom, elements[3]) -- the canvas outside the content is not mapped: it holds these elements as given"""
    chw = _chw(base, planar)
    u8 = M.apply(IDENT if m is None else m, chw)
    if dtype:
        scale, bias = _norm()
        out = np.stack([nm.table(dtype, scale[c], bias[c])[u8[c]] for c in range(3)])
    else:
        out = u8
    if border is not None:
        left, top, right, bottom, el = border
        inside = np.zeros(chw.shape[1:], bool)
        inside[top:chw.shape[1] - bottom, left:chw.shape[2] - right] = True
        for c in range(3):
            out[c][~inside] = el[c]
    return _layout(out, planar)


def same(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype.itemsize == wanted.dtype.itemsize, (what, got.shape, wanted.shape, got.dtype, wanted.dtype)
    bad = np.argwhere(nm.bits(got) != nm.bits(wanted)) if got.dtype != np.uint8 else np.argwhere(got != wanted)
    assert bad.size == 0, (what, "first differing sample", bad[0].tolist(), "differing", len(bad))


def check(ctx, datas, planar, sizes, colours, shape=None, views=None, flags=None, dtype=0, graph=False, border_of=None, pad_value=None, what=""):
    """the request without set_colour as uint8 (once), then with it: statuses equal, every output the model's"""
    base, st0, _ = run(ctx, datas, planar, sizes, shape, None, views, flags)
    outs, st, info = run(ctx, datas, planar, sizes, shape, colours, views, flags, dtype, graph, pad_value)
    assert st == st0
    for k, (o, u, m) in enumerate(zip(outs, base, colours)):
        same(o, want(u, m, planar, dtype, border_of(k) if border_of else None), (what, k, sizes[k], m))
    return base, outs, info


# ---- 1: every element type and layout, every width and height, every matrix ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_bilinear_every_size_and_matrix(ctx, planar, dtype):
    """Four fixtures (one a partial picture), 20 views that walk through widths 1, 3, 5, 37, 259 and heights 1, 7, 9, 33, the eight matrices in
    turn.  The identity views equal the uncoloured bytes; the two saturating matrices give 255 and 0 everywhere."""
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes = sizes_for(20)
    assert {w for w, _ in sizes} == set(WIDTHS) and {h for _, h in sizes} == set(HEIGHTS)
    views = [k % 4 for k in range(20)]
    mats = matrices()
    colours = [mats[k % 8] for k in range(20)]
    base, outs, _ = check(ctx, datas, planar, sizes, colours, views=views, dtype=dtype, what="bilinear")
    if dtype == 0:
        for k, (o, u) in enumerate(zip(outs, base)):
            if colours[k] is IDENT:
                assert np.array_equal(o, u)
            if colours[k] is ALL_HIGH:
                assert (o == 255).all()
            if colours[k] is ALL_LOW:
                assert (o == 0).all()
    assert base[0].dtype == np.uint8


@pytest.mark.parametrize("dtype", [0, nm.DT_BF16], ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
@pytest.mark.parametrize("filt", ["bilinear", "antialias", "bicubic"])
def test_each_filter_with_a_window_and_a_flip(ctx, filt, planar, dtype):
    """The three filters, each from a window of the picture, every other view mirrored; both kernels' ragged tails (37, 259 columns; 7, 9,
    33 rows)."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    dims = [(61, 45), (80, 96), (45, 61)]
    views = [k % 3 for k in range(9)]
    sizes = [(37, 9), (259, 7), (5, 33), (3, 1), (37, 33), (1, 7), (259, 9), (5, 1), (37, 7)]
    wins = []
    for k, p in enumerate(views):
        sw, sh = dims[p]
        tw, th = sizes[k]                                     # the table-driven filters take a window of at most 16x its target on an axis
        wins.append((3 + k % 4, 2 + k % 3, min(sw - 9 - k % 5, 16 * tw), min(sh - 7 - k % 4, 16 * th), 0, 0, 0, 0, k & 1))
    mats = matrices()
    colours = [mats[(k + 1) % 8] for k in range(9)]

    def shape(b):
        b.set_resize_window(wins)
        if filt != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_BICUBIC if filt == "bicubic" else pjd_amd.RESIZE_ANTIALIAS)
    check(ctx, datas, planar, sizes, colours, shape, views, dtype=dtype, what=filt)


@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
@pytest.mark.parametrize("filt", ["bilinear", "antialias"])
def test_each_orientation_once(ctx, filt, planar):
    """The eight orientations in one batch: the row epilogue (1..4) and the transposed one (5..8), full and ragged row tiles."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:2]]
    views = [k % 2 for k in range(8)]
    # the DELIVERED sizes; Q's target (the axes swapped for 5..8) is never less than a sixteenth of the picture: the table-driven filters' limit
    sizes = [(37, 9), (259, 7), (5, 33), (33, 37), (9, 259), (7, 5), (33, 5), (8, 16)]
    mats = matrices()
    colours = [mats[(k + 5) % 8] for k in range(8)]

    def shape(b):
        b.set_orientation(list(range(1, 9)))
        if filt != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
    for dtype in (0, nm.DT_F16):
        check(ctx, datas, planar, sizes, colours, shape, views, dtype=dtype, what=("orientation", filt))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_the_border_of_a_pad_is_not_mapped(ctx, planar, dtype):
    """Letterboxed outputs: the content goes through the map, the border holds the fill as given -- its normalised value, or the pad value
    -- and not its image under the matrix (BGR and the jitters would change it, the saturating matrices erase it)."""
    from pjd_amd import tensors
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0, 1, 2]
    sizes = [(37, 33), (259, 9), (9, 7), (40, 40), (5, 3), (37, 9)]
    pads = [(3, 2, 5, 1), (1, 0, 2, 3), None, (0, 7, 0, 8), (2, 1, 1, 1), (6, 0, 0, 0)]
    mats = matrices()
    colours = [mats[1], mats[3], mats[5], mats[4], mats[6], mats[7]]
    scale, bias = _norm()
    for pad_value in ([None] if dtype == 0 else [None, (0.0, -2.0, 0.5)]):
        if dtype == 0:
            el = FILL
        elif pad_value is None:
            el = [nm.table(dtype, scale[c], bias[c])[FILL[c]] for c in range(3)]
        else:
            v = np.asarray(pad_value, np.float32)          # exact in all three types
            el = list(v.astype(np.float16) if dtype == nm.DT_F16 else nm.to_bf16_bits(v) if dtype == nm.DT_BF16 else v)

        def border_of(k):
            return (*(pads[k] or (0, 0, 0, 0)), el)
        base, outs, _ = check(ctx, datas, planar, sizes, colours, lambda b: b.set_resize_pad(pads, FILL), views, dtype=dtype, border_of=border_of,
                              pad_value=pad_value, what=("pad", pad_value))
        if dtype == 0:                                       # the uncoloured border is the fill, and so is the coloured one: a corner of the first canvas
            for o in (base[0], outs[0]):
                assert tuple(int(v) for v in _chw(o, planar)[:, 0, 0]) == FILL


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_the_affine_warp_and_its_fill(ctx, planar, dtype):
    """Under set_resize_affine the fill takes part in the blend, so it passes through the map: a translated view has a fill band whose
    bytes are the matrix of the fill; a 30 degree rotation; the warp tile's ragged edges (33 = 32 + 1)."""
    from pjd_amd import tensors
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0, 1, 2]
    sizes = [(61, 45), (37, 33), (259, 9), (33, 33), (5, 7), (1, 1)]
    rot = tensors.affine_inverse_matrix((96, 80), (33, 37), angle=30)
    affs = [(1, 0, -7, 0, 1, 5), rot, (0.3, 0.02, 1, -0.01, 5.5, 0.5), (1.3, 0.2, -3, -0.1, 0.8, 2), (1, 0, 1000, 0, 1, -1000), (3, 1, 20, -2, 1, 30)]
    mats = matrices()
    colours = [mats[5], mats[6], mats[1], mats[0], mats[7], mats[2]]
    base, outs, _ = check(ctx, datas, planar, sizes, colours, lambda b: b.set_resize_affine(affs, FILL), views, dtype=dtype, what="warp")
    if dtype == 0:
        band, plain_band = _chw(outs[0], planar)[:, -5:, :7], _chw(base[0], planar)[:, -5:, :7]
        for c in range(3):
            assert (plain_band[c] == FILL[c]).all() and (band[c] == M.value(colours[0], FILL)[c]).all()
        assert M.value(colours[0], FILL) != FILL
        assert (_chw(outs[4], planar) == np.asarray(M.value(colours[4], FILL), np.uint8)[:, None, None]).all()      # wholly outside


# ---- 2: the index is the OUTPUT --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
@pytest.mark.parametrize("form", ["resize", "antialias", "warp"])
def test_seven_views_in_non_monotone_order(ctx, form, planar):
    """Three pictures, seven small views -- several outputs share one workgroup of four tiles -- each with a matrix of its own, two of
    them the identity."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [2, 0, 0, 1, 2, 1, 0]
    sizes = [(5, 7), (37, 9), (4, 3), (9, 7), (37, 7), (7, 9), (5, 3)]      # none less than a sixteenth of its picture (the antialiased filter's limit)
    mats = matrices()
    colours = [mats[5], IDENT, mats[1], mats[6], None, mats[2], mats[7]]
    shape = {"resize": None, "antialias": lambda b: b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS),
             "warp": lambda b: b.set_resize_affine([(1.1, 0.1, 2, -0.1, 0.9, 1)] * 7, FILL)}[form]
    base, outs, info = check(ctx, datas, planar, sizes, colours, shape, views, what=form)
    for k in (1, 4):
        assert np.array_equal(outs[k], base[k])
    assert len({o.tobytes() for o in outs}) == 7


def test_the_record_is_counted_and_the_launches_keep_their_names(ctx):
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    sc = [_scanned(d) for d in datas]
    mats = matrices()
    for warp in (False, True):
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:       # the names of the same batch without the call
            b.set_resize([(9, 37)] * 3)
            if warp:
                b.set_resize_affine([(1, 0, 0, 0, 1, 0)] * 3, FILL)
            b.upload()
            plain_names = list(b.decode_timed()[0])
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_resize([(9, 37)] * 3)
            if warp:
                b.set_resize_affine([(1, 0, 0, 0, 1, 0)] * 3, FILL)
            before = b.info()["device_bytes"]
            b.set_colour(mats[5:8])
            # 64 bytes per output; without an affine map also the windows (40) and canvases (32 + the line prefix) of the padded form
            grown = b.info()["device_bytes"] - before
            assert grown == (3 * 64 if warp else 3 * 64 + 3 * 40 + 3 * 32 + 4 * 4), grown
            b.upload()
            per, _ = b.decode_timed()
            names = list(per)
            assert (names[-1] == "warp" and "resize" not in names) if warp else ("resize" in names and "warp" not in names), names
            assert names == plain_names + ([] if warp else ["pad"]), (names, plain_names)     # no launch of its own: the padded form's two, or the warp's one


# ---- 3: bound output ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_bound_output_at_unaligned_offsets(ctx, planar, dtype):
    """The outputs bound into a donor batch's decoded picture: odd byte offsets (uint8), element-aligned but not vector-aligned ones
    (floats), widths that are no multiple of four.  Every output is the model's, every byte outside them is still the donor's."""
    import pjd_amd
    es = nm.ESIZE[dtype] if dtype else 1
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0, 1, 2]
    sizes = [(37, 9), (259, 7), (5, 33), (3, 7), (1, 1), (37, 33)]
    mats = matrices()
    colours = [mats[5], mats[1], mats[6], mats[0], mats[7], mats[2]]
    oris = [1, 1, 6, 1, 3, 8]                                # both epilogues under the unaligned stores
    base, st0, _ = run(ctx, datas, planar, sizes, lambda b: b.set_orientation(oris), None, views)
    wants = [want(u, m, planar, dtype) for u, m in zip(base, colours)]
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        donor.upload(); donor.decode()
        (pattern,), _ = donor.download()
        pattern = pattern.reshape(-1).copy()
        mem, cap = donor.device_output(0), donor.output_size(0)
        sc = [_scanned(d) for d in datas]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_views(views)
            b.set_resize([(th, tw) for tw, th in sizes])
            b.set_orientation(oris)
            b.set_colour(colours)
            if dtype:
                b.set_normalize(dtype, *_norm())
            offs, pos = [], 7 * es
            for i in range(len(views)):
                while (pos // es) % 4 != (i % 3) + 1:
                    pos += es
                offs.append(pos)
                pos += b.output_size(i) + 5 * es
            assert pos <= cap and all((o // es) % 4 != 0 for o in offs) and (es > 1 or any(o % 2 for o in offs))
            b.bind_output(mem, cap, offs)
            b.upload(); b.decode()
            outs, st = b.download()
            nbytes = [b.output_size(i) for i in range(len(views))]
        (after,), _ = donor.download()
        after = after.reshape(-1)
    assert st == st0
    covered = np.zeros(cap, bool)
    for k, (o, w, off, size) in enumerate(zip(outs, wants, offs, nbytes)):
        same(o, w, (k, sizes[k]))
        assert size == w.nbytes and after[off:off + size].tobytes() == w.tobytes(), k
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every output were written, first at {stray[:8]}"


# ---- 4: repeatability and the other paths into the launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["resize", "bicubic", "warp"])
def test_a_captured_graph_replayed_twice(ctx, form):
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes = [(37, 9), (259, 7), (5, 33), (37, 33)]
    mats = matrices()
    shape = {"resize": None, "bicubic": lambda b: b.set_resize_filter(pjd_amd.RESIZE_BICUBIC), "warp": lambda b: b.set_resize_affine([(1.2, 0.1, 2, -0.1, 0.9, 1)] * 4, FILL)}[form]
    check(ctx, datas, True, sizes, mats[4:8], shape, graph=True, what=("graph", form))


def test_sequential_partial_and_libjpeg_pictures_in_one_batch(ctx):
    """A PJD_F_FORCE_SEQUENTIAL picture, the truncated fixture (a partial picture, grey behind the error) and a PJD_F_LIBJPEG picture in one
    mixed batch; the reduced-size decode of both scale families in front of the resample."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes = [(37, 9), (259, 7), (5, 33), (37, 33)]
    mats = matrices()
    for flags in ([pjd_amd.F_FORCE_SEQUENTIAL, pjd_amd.F_LIBJPEG, 0, 0], [pjd_amd.F_SCALE_1_2, pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_1_2, 0, pjd_amd.F_FORCE_SEQUENTIAL]):
        base, outs, info = check(ctx, datas, True, sizes, mats[4:8], flags=flags, what=("mixed", flags))
        assert info["n_sequential"] >= 1
    _, st, _ = run(ctx, datas, True, sizes, colours=mats[:4])
    assert st[3] != 0 and st[:3] == [0, 0, 0]


def test_the_resample_runs_again_behind_the_exact_kernel_fallback(monkeypatch):
    """A stream of tests/fallback_corpus.py that the parallel decoder hands to the exact kernel in pjd_batch_sync: the first pass mapped a
    picture that was not there yet, so the coloured launch has to run again behind the re-decode."""
    import pjd_amd
    import fallback_corpus as F
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_FORCE_SEQUENTIAL"):
        monkeypatch.delenv(k, raising=False)
    datas = [F.falling()["lock_420_130"].data, golden_bytes("env_61x45_420_q100_opt")]
    views, sizes = [0, 0, 1], [(70, 50), (37, 9), (33, 65)]
    mats = matrices()
    colours = [mats[5], mats[1], mats[6]]
    c = pjd_amd.Context(0)
    try:
        base, st0, info0 = run(c, datas, True, sizes, None, None, views)
        sc = [_scanned(d) for d in datas]
        with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_views(views)
            b.set_resize([(th, tw) for tw, th in sizes])
            b.set_colour(colours)
            b.upload()
            for _ in range(2):
                b.decode(); b.sync()
                outs, st = b.download()
                info = b.info()
                assert info["n_fallback"] == 1 and info["n_sequential"] == 0 and info["sub_bytes"] == 128, info
                assert st == st0
                for k, (o, u, m) in enumerate(zip(outs, base, colours)):
                    same(o, want(u, m, True), ("fallback", k))
    finally:
        c.close()


# ---- 5: call order and arguments ---------------------------------------------------------------------------------------------------------------
def _mats(*ms):
    arr = ((C.c_double * 12) * len(ms))()
    for i, m in enumerate(ms):
        arr[i] = (C.c_double * 12)(*m)
    return arr


def test_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n)) for n in FIXTURES[:2]]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok = _mats(BGR, GRAY)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE                         # before set_resize
        assert b"no resize is set" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
        b.set_resize(sizes)
        assert L.pjd_batch_set_colour(b._h, ok) == 0
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE                         # a second call
        assert b"already set for this batch" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
        # what shapes the resample comes before it
        assert L.pjd_batch_set_resize_filter(b._h, pjd_amd.RESIZE_ANTIALIAS) == E_STATE and b"after set_colour" in L.pjd_last_error(ctx._h)
        assert L.pjd_batch_set_resize_affine(b._h, ((C.c_double * 6) * 2)(), (C.c_uint8 * 3)()) == E_STATE
        assert L.pjd_batch_set_orientation(b._h, (C.c_uint8 * 2)(1, 1)) == E_STATE
        b.upload(); b.decode()                                                      # still a usable batch
        assert b.download()[1] == [0, 0]
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE and b"after set_normalize" in L.pjd_last_error(ctx._h)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0      # which sets the identity resize itself
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE and b"after upload" in L.pjd_last_error(ctx._h)
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_colour(b._h, ok) == E_STATE and b"after bind_output" in L.pjd_last_error(ctx._h)
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_colour(b._h, ok) == E_STATE                         # a BMP batch takes no resize
    for bad in ([BGR], [BGR, BGR[:11]]):
        with pytest.raises(ValueError):
            with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
                b.set_resize(sizes)
                b.set_colour(bad)


def test_argument_errors_name_the_output_and_leave_the_batch_as_it_was(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    datas = [golden_bytes(n) for n in FIXTURES[:2]]
    sc = [_scanned(d) for d in datas]
    descs = [x.desc for x in sc]
    sizes = [(37, 9), (5, 7)]
    bads = [(float("nan"),) + BGR[1:], BGR[:5] + (float("inf"),) + BGR[6:], (16 + 2.0 ** -16,) + BGR[1:], BGR[:3] + (-4096 - 2.0 ** -16,) + BGR[4:], BGR[:10] + (1e300,) + BGR[11:]]
    with ctx.batch(descs, pjd_amd.OUT_GRAY8) as b:
        b.set_resize([(th, tw) for tw, th in sizes])
        assert L.pjd_batch_set_colour(b._h, _mats(BGR, BGR)) == E_ARG and b"grey" in L.pjd_last_error(ctx._h)
    base, st0, _ = run(ctx, datas, False, sizes)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize([(th, tw) for tw, th in sizes])
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_colour(b._h, None) == E_ARG
        for bad in bads:
            assert L.pjd_batch_set_colour(b._h, _mats(GRAY, bad)) == E_ARG, bad
            assert b"picture 1" in L.pjd_last_error(ctx._h), (bad, L.pjd_last_error(ctx._h))
            assert not pjd_amd.colour_check(bad)
        assert L.pjd_batch_set_colour(b._h, _mats(bads[2], GRAY)) == E_ARG and b"picture 0" in L.pjd_last_error(ctx._h)
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                      # after the refused calls: the plain resize
        outs, st = b.download()
    assert st == st0 and all(np.array_equal(o, u) for o, u in zip(outs, base))
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:                                   # with views the text names view and picture; the call stays open
        b.set_views([1, 0, 1])
        b.set_resize([(7, 5)] * 3)
        assert L.pjd_batch_set_colour(b._h, _mats(GRAY, GRAY, bads[0])) == E_ARG
        assert b"view 2 (picture 1)" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
        every = (16, -16, 16, -4096, -16, 16, -16, 4096, 16, 16, -16, -4096)         # every limit met exactly
        b.set_colour([GRAY, every, None])
        b.upload(); b.decode()
        outs, st = b.download()
    base3, _, _ = run(ctx, datas, False, [(5, 7)] * 3, views=[1, 0, 1])
    for o, u, m in zip(outs, base3, (GRAY, every, None)):
        same(o, want(u, m, False), m)


# ---- 6: the torch side, in a child process (tests/colour_torch_cases.py imports torch first) ---------------------------------------------------
def test_tensor_helpers_with_colours():
    """colours= of the two tensor helpers equals the Batch-level result (views, a letterbox, channels_last, bf16), None entries are the
    identity, gray=True and a wrong count raise ValueError."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "colour_torch_cases.py"), "colours"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CASE OK colours" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])
