"""Affine warp on decode (pjd_batch_set_resize_affine) on the GPU (run with -m gpu on an MI355X).  The source P of every case is the
picture the library delivers WITHOUT a resample, downloaded once; every expectation is tests/warp_model.py -- Python integers over
the text of include/pjd.h -- of that P, and every comparison is byte (bit, for floats) equality."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import warp_model as M
from conftest import golden_bytes, ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
FIXTURES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61", "gray_33x70", "err_truncated_eoi_420"]
FMTS = ["rgb8", "planar", "gray"]
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
FILL = (114, 7, 201)
IDENT = (1, 0, 0, 0, 1, 0)
TILE_W, TILE_H = 32, 32                                     # PJD_WARP_COLS x PJD_WARP_ROWS


def _fmt(fmt):
    import pjd_amd
    return {"rgb8": pjd_amd.OUT_RGB8, "planar": pjd_amd.OUT_RGB8_PLANAR, "gray": pjd_amd.OUT_GRAY8}[fmt]


def _scanned(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _chw(a, fmt):
    """a downloaded picture as [C, h, w]"""
    return a.transpose(2, 0, 1) if fmt == "rgb8" else a[None] if fmt == "gray" else a


def _out_layout(chw, fmt):
    return np.ascontiguousarray(chw.transpose(1, 2, 0)) if fmt == "rgb8" else chw[0] if fmt == "gray" else chw


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


_PLAIN = {}


def plain(ctx, data, fmt, flags=0):
    """(status, P as uint8 [C, h, w]): what the batch delivers without a resample.  Decoded once per (stream, format, flags)."""
    key = (data, fmt, flags)
    if key not in _PLAIN:
        sc = _scanned(data, flags)
        with ctx.batch([sc.desc], _fmt(fmt)) as b:
            b.upload(); b.decode()
            (o,), (st,) = b.download()
        p = np.ascontiguousarray(_chw(o, fmt))
        p.setflags(write=False)
        _PLAIN[key] = (st, p)
    return _PLAIN[key]


@functools.lru_cache(maxsize=None)
def one_by_one():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth.make(1, 1, 77, 90, synth.SUB_444)


def case_list(sw, sh, seed):
    """The cases of tools/warp_host.cpp for a source of sw x sh: [(tw, th, matrix)]"""
    rng = np.random.default_rng(seed)
    cases = [(sw, sh, IDENT),
             (sh, sw, (0, -1, sw, 1, 0, 0)), (sh, sw, (0, 1, 0, -1, 0, sh)),       # the two quarter turns
             (sw, sh, (-1, 0, sw, 0, 1, 0)),                                       # a mirror
             (sw, sh, (1, 0, -7, 0, 1, 5)),                                        # a fill band left and at the bottom
             (sw, sh, (1, 0, 0.5, 0, 1, -0.5)),                                    # half a pixel
             (40, 30, (1, 0, 1000, 0, 1, -1000)),                                  # wholly outside
             (1, 1, (3, 1, sw / 3, -2, 1, sh / 2)),                                # a 1 x 1 target
             (TILE_W + 1, TILE_H + 1, (1.3, 0.2, -3, -0.1, 0.8, 2)),               # one pixel past a tile edge on each axis
             (257, 9, (0.33, 0.01, 1, 0.02, 5.5, 0.5))]                            # ... and past the resize tile's
    for _ in range(10):
        tw, th = int(rng.integers(1, 150)), int(rng.integers(1, 80))
        cases.append((tw, th, tuple(M.similarity(rng, sw, sh, tw, th))))
    return cases


def run(ctx, datas, fmt, sizes, mats, views=None, flags=0, dtype=0, fill=FILL, graph=False):
    """One batch in the library's own buffer -> (outputs, statuses, info)."""
    import pjd_amd
    from pjd_amd import tensors
    sc = [_scanned(d, flags) for d in datas]
    with ctx.batch([x.desc for x in sc], _fmt(fmt)) as b:
        if views is not None:
            b.set_views(views)
        b.set_resize([(th, tw) for tw, th in sizes])
        b.set_resize_affine(mats, fill)
        if dtype:
            b.set_normalize(dtype, *tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD))
        b.upload()
        if graph:
            b.capture()
            for _ in range(2):
                b.decode(); b.sync()
        else:
            b.decode()
        outs, st = b.download()
        return outs, st, b.info()


def want_u8(P, m, tw, th, fmt, fill=FILL):
    return _out_layout(M.warp(P, m, tw, th, fill), fmt)


def want_float(P, m, tw, th, fmt, dtype, fill=FILL):
    """pjd_normalize_value of the model's bytes: the 256-entry table of tests/normalize_model.py, per channel"""
    from pjd_amd import tensors
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    u8 = M.warp(P, m, tw, th, fill)
    out = np.stack([nm.table(dtype, scale[c], bias[c])[u8[c]] for c in range(u8.shape[0])])
    return _out_layout(out, fmt)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(nm.bits(got) != nm.bits(want)) if got.dtype != np.uint8 else np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 1: the case list over every fixture, every output format; many views of one picture ------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_case_list_over_every_fixture(ctx, fmt):
    """Every case of tools/warp_host.cpp on the five fixtures and a 1 x 1 picture, all views of ONE batch (each picture decoded once, a
    matrix per view), in all three output formats: byte equality with the model, the statuses those of the plain decode."""
    datas = [golden_bytes(n) for n in FIXTURES] + [one_by_one()]
    src = [plain(ctx, d, fmt) for d in datas]
    assert src[4][0] != 0 and src[5][1].shape[1:] == (1, 1)
    views, sizes, mats = [], [], []
    for p, (_, P) in enumerate(src):
        for tw, th, m in case_list(P.shape[2], P.shape[1], 100 + p):
            views.append(p); sizes.append((tw, th)); mats.append(m)
    outs, st, info = run(ctx, datas, fmt, sizes, mats, views)
    assert st == [s for s, _ in src]
    nc = 1 if fmt == "gray" else 3
    assert info["out_bytes"] == sum(nc * tw * th for tw, th in sizes)
    for k, (o, p, (tw, th), m) in enumerate(zip(outs, views, sizes, mats)):
        same(o, want_u8(src[p][1], m, tw, th, fmt), (k, p, tw, th, m))


def test_without_views_and_the_launch_is_named_warp(ctx):
    """A batch without views; the 48-byte record per output is counted once, the launch is named "warp" and stands in place of "resize";
    a batch that never makes the call names and counts what it did."""
    import pjd_amd
    datas = [golden_bytes(n) for n in FIXTURES]
    src = [plain(ctx, d, "planar") for d in datas]
    rng = np.random.default_rng(3)
    sizes = [(50, 40), (65, 33), (7, 90), (64, 32), (31, 31)]
    mats = [tuple(M.similarity(rng, P.shape[2], P.shape[1], tw, th)) for (_, P), (tw, th) in zip(src, sizes)]
    sc = [_scanned(d) for d in datas]
    for call in (True, False):
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_resize([(th, tw) for tw, th in sizes])
            before = b.info()["device_bytes"]
            if call:
                b.set_resize_affine(mats, FILL)
            assert b.info()["device_bytes"] == before + (48 * len(datas) if call else 0)
            b.upload()
            per, total = b.decode_timed()
            outs, st = b.download()
        assert st == [s for s, _ in src]
        if call:
            assert list(per)[-1] == "warp" and "resize" not in per and "pad" not in per and per["warp"] > 0, per
            for o, (_, P), (tw, th), m in zip(outs, src, sizes, mats):
                same(o, want_u8(P, m, tw, th, "planar"), (tw, th, m))
        else:
            assert list(per)[-1] == "resize" and "warp" not in per, per


# ---- 2: normalised output -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", FMTS)
def test_normalised_output(ctx, fmt, dtype):
    """The three float types in every layout: pjd_normalize_value of the model's bytes, the fill included -- it is a sample like any other."""
    datas = [golden_bytes(n) for n in FIXTURES[:3]]
    src = [plain(ctx, d, fmt) for d in datas]
    views, sizes, mats = [], [], []
    for p, (_, P) in enumerate(src):
        cl = case_list(P.shape[2], P.shape[1], 200 + p)
        for tw, th, m in [cl[0], cl[1], cl[4], cl[6], cl[8], cl[9]] + cl[10:14]:
            views.append(p); sizes.append((tw, th)); mats.append(m)
    outs, st, _ = run(ctx, datas, fmt, sizes, mats, views, dtype=dtype)
    assert st == [0, 0, 0]
    for k, (o, p, (tw, th), m) in enumerate(zip(outs, views, sizes, mats)):
        same(o, want_float(src[p][1], m, tw, th, fmt, dtype), (k, p, tw, th, m))
    # an output wholly outside is the normalised fill and nothing else
    k = next(i for i, m in enumerate(mats) if m[2] == 1000)
    from pjd_amd import tensors
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    chw = _chw(outs[k], fmt)
    for c in range(chw.shape[0]):
        assert (nm.bits(chw[c]) == nm.bits(nm.table(dtype, scale[c], bias[c])[FILL[c]:FILL[c] + 1])[0]).all()


# ---- 3: bound output at odd offsets over two pre-fills: every byte written, none outside --------------------------------------------------------
@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=lambda d: DT_NAME.get(d, "u8"))
@pytest.mark.parametrize("fmt", FMTS)
def test_bound_output_at_odd_offsets_over_two_prefills(ctx, fmt, dtype):
    """The outputs bound into the decoded pictures of two donor batches (two different pre-fills of caller-owned memory), 1, 2 and 3
    elements off a multiple of four, gaps between them as guard bands.  After each decode every output is the model's -- the fill where
    nothing maps, so every byte was written -- and every byte outside the outputs is still the donor's."""
    import pjd_amd
    from pjd_amd import tensors
    es = nm.ESIZE[dtype] if dtype else 1
    # what fits the smaller donor (562 500 bytes) at this element size: the identity, a quarter turn, the fill band, all fill, both tile
    # edges and three general maps of all five fixtures; in 16 bits without the first and the last two; in binary32 of three fixtures
    pick = {1: [0, 2, 4, 6, 8, 9, 10, 11, 12], 2: [2, 4, 6, 8, 9, 10], 4: [2, 4, 6, 8, 9]}[es]
    datas = [golden_bytes(n) for n in (FIXTURES if es < 4 else FIXTURES[:3])]
    src = [plain(ctx, d, fmt) for d in datas]
    views, sizes, mats = [], [], []
    for p, (_, P) in enumerate(src):
        cl = case_list(P.shape[2], P.shape[1], 300 + p)
        for tw, th, m in [cl[k] for k in pick]:
            views.append(p); sizes.append((tw, th)); mats.append(m)
    wants = [(want_float(src[p][1], m, tw, th, fmt, dtype) if dtype else want_u8(src[p][1], m, tw, th, fmt)) for p, (tw, th), m in zip(views, sizes, mats)]
    prefills = []
    for donor_name in ("big_640x480_420_q85", "big_500x375_444_q92_opt"):
        donor_sc = _scanned(golden_bytes(donor_name))
        with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
            donor.upload(); donor.decode()
            (pattern,), _ = donor.download()
            pattern = pattern.reshape(-1).copy()
            mem, cap = donor.device_output(0), donor.output_size(0)
            sc = [_scanned(d) for d in datas]
            with ctx.batch([x.desc for x in sc], _fmt(fmt)) as b:
                b.set_views(views)
                b.set_resize([(th, tw) for tw, th in sizes])
                b.set_resize_affine(mats, FILL)
                if dtype:
                    b.set_normalize(dtype, *tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD))
                offs, pos = [], 7 * es
                for i in range(len(views)):
                    while (pos // es) % 4 != (i % 3) + 1:
                        pos += es
                    offs.append(pos)
                    pos += b.output_size(i) + 5 * es
                assert pos <= cap and sorted({(o // es) % 4 for o in offs}) == [1, 2, 3]
                b.bind_output(mem, cap, offs)
                b.upload(); b.decode()
                outs, st = b.download()
                sizes_b = [b.output_size(i) for i in range(len(views))]
            (after,), _ = donor.download()
            after = after.reshape(-1)
        assert st == [s for s, _ in src]
        covered = np.zeros(cap, bool)
        for k, (o, w, off, size) in enumerate(zip(outs, wants, offs, sizes_b)):
            same(o, w, (k, views[k], sizes[k], mats[k]))
            assert size == w.nbytes and after[off:off + size].tobytes() == w.tobytes(), k
            covered[off:off + size] = True
        stray = np.flatnonzero(~covered & (after != pattern))
        assert stray.size == 0, f"bytes outside every output were written, first at {stray[:8]}"
        prefills.append(pattern[:offs[-1] + sizes_b[-1]])
    assert not np.array_equal(prefills[0], prefills[1]), "the two pre-fills differ"


# ---- 4: the other paths into the launch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["libjpeg", "sequential", "scale_1_2", "graph"])
def test_other_paths_into_the_launch(ctx, mode):
    """A PJD_F_LIBJPEG picture, the exact kernel (PJD_F_FORCE_SEQUENTIAL), a box pre-scale in front, and a captured graph replayed twice."""
    import pjd_amd
    flags = {"libjpeg": pjd_amd.F_LIBJPEG, "sequential": pjd_amd.F_FORCE_SEQUENTIAL, "scale_1_2": pjd_amd.F_SCALE_1_2, "graph": 0}[mode]
    datas = [golden_bytes(n) for n in ("noise_80x96_422_q50_opt", "env_61x45_420_q100_opt", "err_truncated_eoi_420")]
    src = [plain(ctx, d, "planar", flags) for d in datas]
    views, sizes, mats = [], [], []
    for p, (_, P) in enumerate(src):
        cl = case_list(P.shape[2], P.shape[1], 400 + p)
        for tw, th, m in [cl[0], cl[1], cl[8]] + cl[10:14]:
            views.append(p); sizes.append((tw, th)); mats.append(m)
    outs, st, info = run(ctx, datas, "planar", sizes, mats, views, flags=flags, graph=mode == "graph")
    assert st == [s for s, _ in src]
    if mode == "sequential":
        assert info["n_sequential"] == len(datas)
    for k, (o, p, (tw, th), m) in enumerate(zip(outs, views, sizes, mats)):
        same(o, want_u8(src[p][1], m, tw, th, "planar"), (mode, k, p, tw, th, m))


def test_the_warp_runs_again_behind_the_exact_kernel_fallback(monkeypatch):
    """A stream of tests/fallback_corpus.py that the parallel decoder hands to the exact kernel in pjd_batch_sync: the warp of the first
    pass read a picture that was not there yet, so the launch has to run again behind the re-decode."""
    import pjd_amd
    import fallback_corpus as F
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_FORCE_SEQUENTIAL"):
        monkeypatch.delenv(k, raising=False)
    data = F.falling()["lock_420_130"].data
    good = golden_bytes("env_61x45_420_q100_opt")
    c = pjd_amd.Context(0)
    try:
        src = [plain(c, data, "planar"), plain(c, good, "planar")]
        rng = np.random.default_rng(9)
        views, sizes = [0, 0, 1], [(70, 50), (src[0][1].shape[1], src[0][1].shape[2]), (33, 65)]
        mats = [tuple(M.similarity(rng, src[0][1].shape[2], src[0][1].shape[1], 70, 50)), (0, -1, src[0][1].shape[2], 1, 0, 0),
                tuple(M.similarity(rng, 61, 45, 33, 65))]
        sc = [_scanned(data), _scanned(good)]
        with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_views(views)
            b.set_resize([(th, tw) for tw, th in sizes])
            b.set_resize_affine(mats, FILL)
            b.upload()
            for _ in range(2):
                b.decode(); b.sync()
                outs, st = b.download()
                info = b.info()
                assert info["n_fallback"] == 1 and info["n_sequential"] == 0 and info["sub_bytes"] == 128, info
                assert st == [src[0][0], src[1][0]]
                for o, p, (tw, th), m in zip(outs, views, sizes, mats):
                    same(o, want_u8(src[p][1], m, tw, th, "planar"), (p, tw, th))
    finally:
        c.close()
        _PLAIN.pop((data, "planar", 0), None); _PLAIN.pop((good, "planar", 0), None)      # they belong to the closed context's settings


def test_a_65535_wide_picture_warped_to_224(ctx):
    """One 65535-wide member of tests/geometry_corpus.py to 224 x 224: the far end of the row at the largest scale the limits allow (16
    source pixels a step, the last source column among the taps), a rotation about a point 65000 pixels in, and a mirror of the far end:
    source coordinates and byte offsets beyond 2^16."""
    import geometry_corpus as G
    name = "w65535x8_444"
    data = G.jpeg(name)
    st0, P = plain(ctx, data, "planar", G.flags(name))
    assert P.shape == (3, 8, 65535) and st0 == 0
    a = np.deg2rad(30)
    # the first map: u - 1/2 = 16 * i + 61982 -- column 222 reads source column 65534, the last one, with weight 0 on the tap beside it; column 223 is outside
    mats = [(16, 0, 61974.5, 0, 8 / 224, 0),
            (np.cos(a) * 2, -np.sin(a) * 2, 65000 - 224 * (np.cos(a) - np.sin(a)), np.sin(a) * 0.05, np.cos(a) * 0.05, 4 - 112 * 0.05 * (np.sin(a) + np.cos(a))),
            (-1, 0, 65535, 0, 1 / 28, 0)]
    outs, st, _ = run(ctx, [data], "planar", [(224, 224)] * 3, mats, [0, 0, 0], flags=G.flags(name))
    assert st == [0]
    for k, (o, m) in enumerate(zip(outs, mats)):
        w = want_u8(P, m, 224, 224, "planar")
        assert k != 0 or ((w[:, :, -1] == np.asarray(FILL)[:, None]).all() and not (w[:, :, 0] == np.asarray(FILL)[:, None]).all()), "the first map runs off the right edge"
        same(o, w, (k, m))


# ---- 5: call order and arguments -----------------------------------------------------------------------------------------------------------
def _mats(*ms):
    arr = ((C.c_double * 6) * len(ms))()
    for i, m in enumerate(ms):
        arr[i] = (C.c_double * 6)(*m)
    return arr


def test_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n)) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok, fill = _mats(IDENT, (0.5, 0.1, 3, -0.1, 0.5, 2)), (C.c_uint8 * 3)(*FILL)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.pjd_batch_set_resize_affine(None, ok, fill) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE                # no resize is set
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == 0
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE                # twice
        # ... and the four it excludes are refused behind it
        assert L.pjd_batch_set_resize_pad(b._h, (pjd_amd.ResizePad * 2)(), fill) == E_STATE
        assert b"set_resize_affine" in L.pjd_last_error(ctx._h)
        assert L.pjd_batch_set_orientation(b._h, (C.c_uint8 * 2)(1, 1)) == E_STATE
        assert L.pjd_batch_set_resize_window(b._h, (pjd_amd.ResizeWindow * 2)()) == E_STATE
        assert L.pjd_batch_set_resize_filter(b._h, pjd_amd.RESIZE_BILINEAR) == E_STATE
        assert L.pjd_batch_set_views(b._h, (C.c_uint32 * 2)(0, 1), 2) == E_STATE         # views come first
        b.upload(); b.decode()                                                         # still a usable batch
        assert b.download()[1] == [0, 0]
    # on a batch that took one of the four, in whichever form
    others = [lambda b: b.set_resize_pad([None, None]), lambda b: b.set_resize_pad([(1, 1, 1, 1), None]), lambda b: b.set_orientation([1, 1]),
              lambda b: b.set_orientation([6, 1]), lambda b: b.set_resize_window([None, None]), lambda b: b.set_resize_filter(pjd_amd.RESIZE_BILINEAR),
              lambda b: b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)]
    for k, other in enumerate(others):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            other(b)
            assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE, k
            assert b"exclude" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
            assert L.pjd_batch_set_resize_affine(b._h, None, fill) == E_STATE, k       # the state is judged first
            b.upload(); b.decode()
            assert b.download()[1] == [0, 0]
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE                # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0          # which sets the identity resize itself
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE
    for step in ("upload", "capture", "decode"):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.upload()
            if step == "capture":
                b.capture()
            if step == "decode":
                b.decode()
            assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE, step
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE            # after bind_output
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_resize_affine(b._h, ok, fill) == E_STATE                # a BMP batch takes no resize
    for bad in (dict(matrices=[IDENT]), dict(matrices=[IDENT, IDENT], fill=(0, 0)), dict(matrices=[IDENT, IDENT], fill=(0, 0, 256)), dict(matrices=[IDENT, (1, 2, 3)])):
        with pytest.raises(ValueError):
            with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
                b.set_resize(sizes)
                b.set_resize_affine(**bad)


def test_argument_errors_name_the_output_and_leave_the_batch_as_it_was(ctx):
    import pjd_amd
    import resize_model
    L = pjd_amd.dev_lib()
    names = ["gray_33x70", "env_61x45_420_q100_opt"]
    datas = [golden_bytes(n) for n in names]
    src = [plain(ctx, d, "rgb8") for d in datas]
    sc = [_scanned(d) for d in datas]
    sizes = [(31, 17), (20, 30)]
    fill = (C.c_uint8 * 3)(*FILL)
    good = (0.5, 0.1, 3, -0.1, 0.5, 2)
    bads = [(float("nan"), 0, 0, 0, 1, 0), (1, float("inf"), 0, 0, 1, 0), (16 + 2.0 ** -40, 0, 0, 0, 1, 0), (1, 0, 0, -16.5, 1, 0), (1, 0, 262144.5, 0, 1, 0), (1, 0, 0, 0, 1, -1e9)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_resize_affine(b._h, None, fill) == E_ARG
        assert L.pjd_batch_set_resize_affine(b._h, _mats(good, good), None) == E_ARG
        for bad in bads:
            assert L.pjd_batch_set_resize_affine(b._h, _mats(good, bad), fill) == E_ARG, bad
            assert b"picture 1" in L.pjd_last_error(ctx._h), (bad, L.pjd_last_error(ctx._h))
            assert not pjd_amd.resize_affine_check(61, 45, 30, 20, bad)
        assert L.pjd_batch_set_resize_affine(b._h, _mats(bads[2], good), fill) == E_ARG and b"picture 0" in L.pjd_last_error(ctx._h)
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                         # after the refused calls: the plain resize
        outs, st = b.download()
    assert st == [0, 0]
    for (_, P), (th, tw), o in zip(src, sizes, outs):
        assert np.array_equal(o, resize_model.resize(P.transpose(1, 2, 0), tw, th))
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:                       # with views the text names view and picture; the call stays open
        b.set_views([1, 0, 1])
        b.set_resize([(20, 30)] * 3)
        assert L.pjd_batch_set_resize_affine(b._h, _mats(good, good, bads[0]), fill) == E_ARG
        assert b"view 2 (picture 1)" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
        every = (16, -16, 262144, -16, 16, -262144)                                    # every limit met exactly
        b.set_resize_affine([good, every, IDENT], FILL)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0, 0]
    for o, p, m in zip(outs, (1, 0, 1), (good, every, IDENT)):
        same(o, want_u8(src[p][1], m, 30, 20, "rgb8"), m)


# ---- 6: the torch side, in a child process (tests/warp_torch_cases.py imports torch first) -----------------------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "warp_torch_cases.py"), case] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_tensor_helpers_with_affines():
    """affines= of the two tensor helpers: angle=90 is numpy.rot90(P, 1), angle=0 with scale=1 is P, orientation 6 with the identity map is
    orientations= alone, channels_last and gray=True against the model, views, the keywords it excludes."""
    _torch_case("affines")
