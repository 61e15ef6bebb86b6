"""Gaussian blur on decode (pjd_batch_set_blur) on the GPU (run with -m gpu on an MI355X).  The expectation of every case is
tests/blur_model.py -- integers over the text of include/pjd.h, the taps from pjd_blur_taps -- applied to what the SAME batch delivers as
uint8 WITHOUT set_blur, downloaded once per request; normalised cases put tests/normalize_model.py on top.  Every comparison is byte
(bit, for floats) equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import blur_model as M
import colour_model as CM
import normalize_model as nm
from conftest import golden_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
FIXTURES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61", "err_truncated_eoi_420"]
DTYPES = [0, nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
WIDTHS, HEIGHTS = (1, 2, 5, 37, 259), (1, 7, 9, 33, 70)
BLURS = [None, (1, 1.0), (3, 0.1), (3, 0.8), (23, 2.0), (63, 10.0), (5, 100.0)]
FILL = (114, 7, 201)
RECORD, PREFIX = 40, 4                                       # bytes: one PjdDevBlur per output, one prefix word per output and one more


def sizes_and_blurs():
    """20 views (tw, th) over every width and every height, the seven entries in turn, shifted so that 63 taps meet widths 1 and 2"""
    sizes = [(WIDTHS[k % 5], HEIGHTS[(k + k // 5) % 5]) for k in range(20)]
    blurs = [BLURS[(k + 5 + k // 5) % 7] for k in range(20)]
    return sizes, blurs


def _fmt(planar, gray=False):
    import pjd_amd
    return pjd_amd.OUT_GRAY8 if gray else pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _scanned(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _norm():
    from pjd_amd import tensors
    return tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


def run(ctx, datas, planar, sizes, shape=None, blurs=None, views=None, flags=None, dtype=0, graph=False, gray=False):
    """One batch in the library's own buffer -> (outputs, statuses, info).  shape(b): the setter calls between set_resize and set_blur."""
    flags = flags or [0] * len(datas)
    sc = [_scanned(d, f) for d, f in zip(datas, flags)]
    with ctx.batch([x.desc for x in sc], _fmt(planar, gray)) as b:
        if views is not None:
            b.set_views(views)
        b.set_resize([(th, tw) for tw, th in sizes])
        if shape is not None:
            shape(b)
        if blurs is not None:
            b.set_blur(blurs)
        if dtype:
            b.set_normalize(dtype, *_norm())
        b.upload()
        if graph:
            b.capture()
            for _ in range(2):
                b.decode(); b.sync()
        else:
            b.decode()
        outs, st = b.download()
        return outs, st, b.info()


def want(base, entry, size, planar, dtype=0, gray=False):
    """the model's output for one unblurred uint8 output `base` of size (tw, th): the blur, then the normalisation table per channel, in
    the shape the batch delivers"""
    tw, th = size
    chw = base.reshape(1, th, tw) if gray else base if planar else base.transpose(2, 0, 1)
    u8 = M.blur(chw, entry)
    if dtype:
        scale, bias = _norm()
        out = np.stack([nm.table(dtype, scale[c], bias[c])[u8[c]] for c in range(u8.shape[0])])
    else:
        out = u8
    return (out if gray or planar else np.ascontiguousarray(out.transpose(1, 2, 0))).reshape(base.shape)


def same(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype.itemsize == wanted.dtype.itemsize, (what, got.shape, wanted.shape, got.dtype, wanted.dtype)
    bad = np.argwhere(nm.bits(got) != nm.bits(wanted)) if got.dtype != np.uint8 else np.argwhere(got != wanted)
    assert bad.size == 0, (what, "first differing sample", bad[0].tolist(), "differing", len(bad))


def check(ctx, datas, planar, sizes, blurs, shape=None, views=None, flags=None, dtype=0, graph=False, gray=False, what=""):
    """the request without set_blur as uint8 (once), then with it: statuses equal, every output the model's"""
    base, st0, _ = run(ctx, datas, planar, sizes, shape, None, views, flags, gray=gray)
    outs, st, info = run(ctx, datas, planar, sizes, shape, blurs, views, flags, dtype, graph, gray)
    assert st == st0 and len(outs) == len(blurs)
    for k, (o, u, e) in enumerate(zip(outs, base, blurs)):
        same(o, want(u, e, sizes[k], planar, dtype, gray), (what, k, sizes[k], e))
    return base, outs, info


# ---- 1: sizes and taps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_every_size_and_tap_count(ctx, planar, dtype):
    """Four fixtures (one a partial picture), 20 views over widths 1, 2, 5, 37, 259 and heights 1, 7, 9, 33, 70, the seven entries in turn:
    None and the identity tables equal the base bytes; 63 taps meet a width of 1 and a width of 2 (a halo that folds many times)."""
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes, blurs = sizes_and_blurs()
    assert {w for w, _ in sizes} == set(WIDTHS) and {h for _, h in sizes} == set(HEIGHTS) and set(blurs) == set(BLURS)
    assert {w for (w, _), e in zip(sizes, blurs) if e == (63, 10.0)} >= {1, 2}
    views = [k % 4 for k in range(20)]
    base, outs, _ = check(ctx, datas, planar, sizes, blurs, views=views, dtype=dtype, what="sizes")
    if dtype == 0:
        for o, u, e in zip(outs, base, blurs):
            if e in (None, (1, 1.0), (3, 0.1)):
                assert np.array_equal(o, u), e
        assert any(not np.array_equal(o, u) for o, u in zip(outs, base))
    assert base[0].dtype == np.uint8


# ---- 2: composition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
@pytest.mark.parametrize("filt", ["bilinear", "antialias", "bicubic"])
def test_behind_each_filter_with_a_window_and_a_flip(ctx, filt, planar):
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    dims = [(61, 45), (80, 96), (45, 61)]
    views = [k % 3 for k in range(6)]
    sizes = [(37, 9), (259, 7), (5, 33), (70, 33), (37, 70), (2, 7)]
    wins = []
    for k, p in enumerate(views):
        sw, sh = dims[p]
        tw, th = sizes[k]                                     # the table-driven filters take a window of at most 16x its target on an axis
        wins.append((3 + k % 4, 2 + k % 3, min(sw - 9 - k % 5, 16 * tw), min(sh - 7 - k % 4, 16 * th), 0, 0, 0, 0, k & 1))
    blurs = [(23, 2.0), (5, 100.0), None, (63, 10.0), (3, 0.8), (23, 2.0)]

    def shape(b):
        b.set_resize_window(wins)
        if filt != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_BICUBIC if filt == "bicubic" else pjd_amd.RESIZE_ANTIALIAS)
    check(ctx, datas, planar, sizes, blurs, shape, views, dtype=nm.DT_BF16 if planar else 0, what=filt)


@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_behind_the_eight_orientations(ctx, planar):
    """The delivered sizes are the blur's: a transposed output is blurred upright, over out_w x out_h."""
    datas = [golden_bytes(n) for n in FIXTURES[:2]]
    views = [k % 2 for k in range(8)]
    sizes = [(37, 9), (259, 7), (5, 33), (33, 37), (9, 70), (7, 5), (33, 5), (8, 16)]
    blurs = [(23, 2.0), (3, 0.8), (63, 10.0), None, (5, 100.0), (23, 2.0), (3, 0.8), (63, 10.0)]
    check(ctx, datas, planar, sizes, blurs, lambda b: b.set_orientation(list(range(1, 9))), views, dtype=0 if planar else nm.DT_F16, what="orientation")


@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_behind_the_affine_warp_and_its_fill(ctx, planar):
    """The fill is part of U: a translated view's fill band is blurred into the picture beside it; a view wholly outside stays the fill."""
    from pjd_amd import tensors
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0, 1]
    sizes = [(61, 45), (37, 33), (259, 9), (33, 33), (5, 7)]
    rot = tensors.affine_inverse_matrix((96, 80), (33, 37), angle=30)
    affs = [(1, 0, -7, 0, 1, 5), rot, (0.3, 0.02, 1, -0.01, 5.5, 0.5), (1.3, 0.2, -3, -0.1, 0.8, 2), (1, 0, 1000, 0, 1, -1000)]
    blurs = [(23, 2.0), (63, 10.0), (3, 0.8), None, (23, 2.0)]
    base, outs, _ = check(ctx, datas, planar, sizes, blurs, lambda b: b.set_resize_affine(affs, FILL), views, dtype=0, what="warp")
    chw = outs[4] if planar else outs[4].transpose(2, 0, 1)
    assert (chw == np.asarray(FILL, np.uint8)[:, None, None]).all()                 # a constant picture stays constant
    check(ctx, datas, planar, sizes, blurs, lambda b: b.set_resize_affine(affs, FILL), views, dtype=nm.DT_F32, what="warp f32")


@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_the_blur_reads_the_mapped_bytes(ctx, planar):
    """Behind set_colour: the base is the COLOURED batch, and it differs from the plain one (BGR) or is saturated (all 255)."""
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0]
    sizes = [(37, 33), (70, 9), (5, 7), (64, 32)]
    bgr, high = CM.permutation((2, 1, 0)), (16.0, 16.0, 16.0, 4096.0) * 3
    colours = [bgr, high, None, bgr]
    blurs = [(23, 2.0), (63, 10.0), (3, 0.8), (5, 100.0)]
    plain, _, _ = run(ctx, datas, planar, sizes, None, None, views)
    base, outs, _ = check(ctx, datas, planar, sizes, blurs, lambda b: b.set_colour(colours), views, dtype=0, what="colour")
    assert not np.array_equal(base[0], plain[0]) and (base[1] == 255).all() and (outs[1] == 255).all()
    check(ctx, datas, planar, sizes, blurs, lambda b: b.set_colour(colours), views, dtype=nm.DT_BF16, what="colour bf16")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
def test_grey_batches(ctx, dtype):
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [0, 1, 2, 0, 1]
    sizes = [(37, 33), (259, 9), (1, 7), (70, 70), (2, 1)]
    blurs = [(23, 2.0), (63, 10.0), (3, 0.8), (5, 100.0), None]
    check(ctx, datas, True, sizes, blurs, None, views, dtype=dtype, gray=True, what="grey")


# ---- 3: the index is the OUTPUT ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True], ids=["rgb8", "planar"])
def test_seven_views_in_non_monotone_order(ctx, planar):
    """Three pictures, seven small views with None entries among blurred ones, each record and tap row its own output's."""
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    views = [2, 0, 0, 1, 2, 1, 0]
    sizes = [(5, 7), (37, 9), (4, 3), (9, 7), (37, 7), (7, 9), (5, 3)]
    blurs = [(3, 0.8), None, (23, 2.0), (5, 100.0), None, (63, 10.0), (23, 2.0)]
    base, outs, _ = check(ctx, datas, planar, sizes, blurs, None, views, what="mixed")
    for k in (1, 4):
        assert np.array_equal(outs[k], base[k])
    assert len({o.tobytes() for o in outs}) == 7


# ---- 4: bound output ---------------------------------------------------------------------------------------------------------------------
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
    blurs = [(23, 2.0), (3, 0.8), (63, 10.0), None, (5, 100.0), (23, 2.0)]
    base, st0, _ = run(ctx, datas, planar, sizes, None, None, views)
    wants = [want(u, e, s, planar, dtype) for u, e, s in zip(base, blurs, sizes)]
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
            b.set_blur(blurs)
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


# ---- 5: repeatability and the other paths into the launch --------------------------------------------------------------------------------
def test_a_captured_graph_replayed_twice(ctx):
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes = [(37, 9), (259, 7), (5, 33), (70, 33)]
    check(ctx, datas, True, sizes, [(23, 2.0), (63, 10.0), None, (3, 0.8)], graph=True, dtype=nm.DT_BF16, what="graph")


def test_sequential_partial_and_libjpeg_pictures_in_one_batch(ctx):
    """A PJD_F_FORCE_SEQUENTIAL picture, the truncated fixture (a partial picture) and a PJD_F_LIBJPEG picture in one mixed batch; the
    reduced-size decode of both scale families in front of the resample."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES]
    sizes = [(37, 9), (259, 7), (5, 33), (37, 33)]
    blurs = [(23, 2.0), (3, 0.8), (63, 10.0), (5, 100.0)]
    for flags in ([pjd_amd.F_FORCE_SEQUENTIAL, pjd_amd.F_LIBJPEG, 0, 0], [pjd_amd.F_SCALE_1_2, pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_1_2, 0, pjd_amd.F_FORCE_SEQUENTIAL]):
        base, outs, info = check(ctx, datas, True, sizes, blurs, flags=flags, what=("mixed", flags))
        assert info["n_sequential"] >= 1
    _, st, _ = run(ctx, datas, True, sizes, blurs=blurs)
    assert st[3] != 0 and st[:3] == [0, 0, 0]


def test_the_blur_runs_again_behind_the_exact_kernel_fallback(monkeypatch):
    """A stream of tests/fallback_corpus.py that the parallel decoder hands to the exact kernel in pjd_batch_sync: the first pass blurred a
    picture that was not there yet, so the resample and the blur have to run again behind the re-decode."""
    import pjd_amd
    import fallback_corpus as F
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_FORCE_SEQUENTIAL"):
        monkeypatch.delenv(k, raising=False)
    datas = [F.falling()["lock_420_130"].data, golden_bytes("env_61x45_420_q100_opt")]
    views, sizes = [0, 0, 1], [(70, 50), (37, 9), (33, 65)]
    blurs = [(23, 2.0), None, (63, 10.0)]
    c = pjd_amd.Context(0)
    try:
        base, st0, info0 = run(c, datas, True, sizes, None, None, views)
        sc = [_scanned(d) for d in datas]
        with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_views(views)
            b.set_resize([(th, tw) for tw, th in sizes])
            b.set_blur(blurs)
            b.upload()
            for _ in range(2):
                b.decode(); b.sync()
                outs, st = b.download()
                info = b.info()
                assert info["n_fallback"] == 1 and info["n_sequential"] == 0 and info["sub_bytes"] == 128, info
                assert st == st0
                for k, (o, u, e) in enumerate(zip(outs, base, blurs)):
                    same(o, want(u, e, sizes[k], True), ("fallback", k))
    finally:
        c.close()


def test_poisoned_device_memory_changes_nothing(monkeypatch):
    """Every allocation of a fresh context filled with 0xA5, then with 0x00, before anything touches it -- the blur intermediate, the
    records and the tap table among them: equal outputs, and the model's."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    sizes = [(37, 33), (259, 9), (5, 70)]
    blurs = [(23, 2.0), None, (63, 10.0)]
    got = {}
    for byte in ("0xA5", "0x00"):
        monkeypatch.setenv("PJD_DEBUG_POISON", byte)
        c = pjd_amd.Context(0)
        try:
            base, st0, _ = run(c, datas, True, sizes)
            got[byte], st, _ = run(c, datas, True, sizes, blurs=blurs, dtype=nm.DT_F16)
            assert st == st0
            for k, (o, u, e) in enumerate(zip(got[byte], base, blurs)):
                same(o, want(u, e, sizes[k], True, nm.DT_F16), (byte, k))
        finally:
            c.close()
    for a, b in zip(got["0xA5"], got["0x00"]):
        assert a.tobytes() == b.tobytes()


# ---- 6: accounting -----------------------------------------------------------------------------------------------------------------------
def test_the_launch_is_named_and_everything_is_counted(ctx):
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    sc = [_scanned(d) for d in datas]
    sizes = [(9, 37), (33, 70), (7, 5)]                      # (th, tw)
    blurs = [(23, 2.0), None, (23, 2.0)]                     # one shared row of 23 taps behind row 0
    buf = sum((3 * h * w + 255) & ~255 for h, w in sizes)    # the packed uint8 layout, 256-byte aligned
    for warp in (False, True):
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:       # the names of the same batch without the call
            b.set_resize(sizes)
            if warp:
                b.set_resize_affine([(1, 0, 0, 0, 1, 0)] * 3, FILL)
            b.upload()
            plain_names = list(b.decode_timed()[0])
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_resize(sizes)
            if warp:
                b.set_resize_affine([(1, 0, 0, 0, 1, 0)] * 3, FILL)
            before = b.info()["device_bytes"]
            b.set_blur(blurs)
            grown = b.info()["device_bytes"] - before
            assert grown == buf + 3 * RECORD + 4 * PREFIX + (1 + 23) * 4, (grown, buf)
            b.upload()
            names = list(b.decode_timed()[0])
            assert names == plain_names + ["blur"] and names[-2] == ("warp" if warp else "resize"), (names, plain_names)


# ---- 7: call order and arguments ---------------------------------------------------------------------------------------------------------
def _blurs(*entries):
    import pjd_amd
    arr = (pjd_amd.Blur * len(entries))()
    for i, e in enumerate(entries):
        arr[i] = pjd_amd.Blur(float(e[1]), int(e[0]), int(e[2]) if len(e) > 2 else 0)
    return arr


def test_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n)) for n in FIXTURES[:2]]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok = _blurs((23, 2.0), (0, 0.0))
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    err = lambda: L.pjd_last_error(ctx._h)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE and b"no resize is set" in err(), err()       # before set_resize
        b.set_resize(sizes)
        assert L.pjd_batch_set_blur(b._h, ok) == 0
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE and b"already set for this batch" in err(), err()
        # what shapes the resample comes before it
        assert L.pjd_batch_set_resize_filter(b._h, pjd_amd.RESIZE_ANTIALIAS) == E_STATE and b"after set_blur" in err(), err()
        assert L.pjd_batch_set_resize_affine(b._h, ((C.c_double * 6) * 2)(), (C.c_uint8 * 3)()) == E_STATE and b"after set_blur" in err()
        assert L.pjd_batch_set_orientation(b._h, (C.c_uint8 * 2)(1, 1)) == E_STATE and b"after set_blur" in err()
        assert L.pjd_batch_set_resize_window(b._h, (pjd_amd.ResizeWindow * 2)()) == E_STATE and b"after set_blur" in err()
        assert L.pjd_batch_set_colour(b._h, ((C.c_double * 12) * 2)()) == E_STATE and b"after set_blur" in err()
        assert L.pjd_batch_set_resize_pad(b._h, (pjd_amd.ResizePad * 2)(), (C.c_uint8 * 3)()) == E_STATE and b"after set_blur" in err()
        b.upload(); b.decode()                                                      # still a usable batch
        assert b.download()[1] == [0, 0]
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE and b"after set_normalize" in err(), err()
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0      # which sets the identity resize itself
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE and b"after upload" in err(), err()
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_blur(b._h, ok) == E_STATE and b"after bind_output" in err(), err()
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_blur(b._h, ok) == E_STATE                           # a BMP batch takes no resize
    with pytest.raises(ValueError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_blur([(3, 1.0)])


def test_argument_errors_name_the_output_and_leave_the_batch_as_it_was(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    datas = [golden_bytes(n) for n in FIXTURES[:2]]
    sc = [_scanned(d) for d in datas]
    descs = [x.desc for x in sc]
    sizes = [(37, 9), (5, 7)]
    err = lambda: L.pjd_last_error(ctx._h)
    bads = [(4, 1.0), (64, 1.0), (65, 1.0), (3, float("nan")), (3, float("inf")), (3, 0.0), (3, -2.0), (0, 0.5), (3, 1.0, 1), (0, 0.0, 9)]
    base, st0, _ = run(ctx, datas, False, sizes)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize([(th, tw) for tw, th in sizes])
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_blur(b._h, None) == E_ARG
        for bad in bads:
            assert L.pjd_batch_set_blur(b._h, _blurs((23, 2.0), bad)) == E_ARG, bad
            assert b"picture 1" in err(), (bad, err())
            assert not pjd_amd.blur_check(*bad)
        assert L.pjd_batch_set_blur(b._h, _blurs(bads[0], (23, 2.0))) == E_ARG and b"picture 0" in err()
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                      # after the refused calls: the plain resize
        outs, st = b.download()
    assert st == st0 and all(np.array_equal(o, u) for o, u in zip(outs, base))
    # pad, in both orders: the blur is refused behind it (the batch stays the padded one), and the pad behind the blur by the call order
    pads = [(3, 2, 5, 1), (1, 0, 0, 3)]
    pbase, _, _ = run(ctx, datas, False, sizes, lambda b: b.set_resize_pad(pads, FILL))
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize([(th, tw) for tw, th in sizes])
        b.set_resize_pad(pads, FILL)
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_blur(b._h, _blurs((23, 2.0), (3, 0.8))) == E_ARG and b"set_resize_pad" in err(), err()
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()
        outs, _ = b.download()
    assert all(np.array_equal(o, u) for o, u in zip(outs, pbase))
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize([(th, tw) for tw, th in sizes])
        b.set_blur([(23, 2.0), (3, 0.8)])
        assert L.pjd_batch_set_resize_pad(b._h, (pjd_amd.ResizePad * 2)(), (C.c_uint8 * 3)()) != 0 and b"set_blur" in err(), err()
        b.upload(); b.decode()
        outs, _ = b.download()
    for k, (o, u, e) in enumerate(zip(outs, base, [(23, 2.0), (3, 0.8)])):
        same(o, want(u, e, sizes[k], False), ("pad refused behind the blur", k))
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:                                   # with views the text names view and picture; the call stays open
        b.set_views([1, 0, 1])
        b.set_resize([(7, 5)] * 3)
        assert L.pjd_batch_set_blur(b._h, _blurs((3, 1.0), (3, 1.0), bads[0])) == E_ARG
        assert b"view 2 (picture 1)" in err(), err()
        b.set_blur([(63, 1e308), None, (1, 5e-324)])                                # every limit met
        b.upload(); b.decode()
        outs, st = b.download()
    base3, _, _ = run(ctx, datas, False, [(5, 7)] * 3, views=[1, 0, 1])
    for o, u, e in zip(outs, base3, [(63, 1e308), None, (1, 5e-324)]):
        same(o, want(u, e, (5, 7), False), e)


# ---- 8: the torch side, in a child process (tests/blur_torch_cases.py imports torch first) -----------------------------------------------
def test_tensor_helpers_with_blurs():
    """blurs= of the two tensor helpers equals the Batch-level result (views, channels_last, bf16), None entries are copies, and the uint8
    result is within 1 level of torch's conv2d over the reflect-padded float64 tensor wherever r < min(H, W)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "blur_torch_cases.py"), "blurs"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CASE OK blurs" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])
