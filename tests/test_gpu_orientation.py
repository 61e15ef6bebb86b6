"""Orientation on decode (pjd_batch_set_orientation) on the GPU (run with -m gpu on an MI355X).  Every expectation is
tests/orientation_model.py -- the window model over Q's target, then the three numpy steps of include/pjd.h's table -- over the
oracle's picture, and every comparison is byte (bit, for floats) equality; never something this library delivered.  Every batch
holds all eight orientations, so the launch under test is the mixed one.  The fixtures assert on the CPU, before anything runs on the
device, that no expectation is also what a wrong implementation (orientation ignored, transpose without mirrors, 6 and 8 exchanged,
mirrors before the transpose, the window resolved against the unswapped target) would deliver."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import orientation_model as om
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

# (source (w, h, seed) of a synthetic picture without symmetry, (tw, th) of Q)
#   (259, 13): crosses the 256-column tile, the last lane group has 3 columns, the second row tile 5 rows (a ragged 8-pack); transposed,
#              D's rows are 13 samples long, so the 8-sample stores start at every alignment
#   (5, 259):  33 row tiles, the last one ragged;  (8, 8): one full 8-pack;  (1, 1), (1, 9), (9, 1): one sample, one column, one row
SHAPES = [((600, 40, 51), (259, 13)), ((40, 600, 52), (5, 259)), ((61, 45, 53), (8, 8)),
          ((16, 12, 54), (1, 1)), ((16, 12, 54), (1, 9)), ((16, 12, 54), (9, 1))]


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _filter(b, filt):
    import pjd_amd
    if filt != "bilinear":
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if filt == "antialias" else pjd_amd.RESIZE_BICUBIC)


def _layout(pic, planar):
    return np.ascontiguousarray(pic.transpose(2, 0, 1)) if planar else pic


def _delivered(tw, th, o):
    """(out_h, out_w) to hand to set_resize for Q's target tw x th."""
    return (tw, th) if o >= 5 else (th, tw)


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
def sources(port):
    """{(w, h, seed): (jpeg bytes, the oracle's picture)}"""
    synth = _synth()
    out = {}
    for key in sorted({s for s, _ in SHAPES} | {(61, 45, 53)}):
        data = synth.make(key[0], key[1], key[2], 90, synth.SUB_444)
        out[key] = (data, port.decode(data)["rgb"])
    return out


def _case(rgb, win, tw, th, o, filt, met, what):
    """The expectation for Q's target tw x th in orientation o, checked against the wrong models where the picture has no axis of one
    sample (such a picture is its own mirror image along that axis, and 1 x 1 its own transpose)."""
    out_h, out_w = _delivered(tw, th, o)
    want = om.oriented(rgb, win, out_w, out_h, o, filt)
    if min(tw, th) > 1:
        met |= om.assert_not_a_wrong_model(rgb, win, out_w, out_h, o, filt, want, what)
    return want


@pytest.fixture(scope="module")
def shape_cases(sources):
    """[(jpeg, (out_h, out_w), o, {filter: expectation})]: every shape in every orientation, 48 pictures."""
    out, met = [], set()
    for src, (tw, th) in SHAPES:
        data, rgb = sources[src]
        for o in ORIS:
            out.append((data, _delivered(tw, th, o), o, {f: _case(rgb, None, tw, th, o, f, met, (src, tw, th, o, f)) for f in FILTERS}))
    assert met == {"ignored", "no_mirrors", "exchanged_6_8", "mirrors_first"}, met
    return out


def _run(ctx, cases, planar, filt, dtype=0, wins=None, flags=0):
    """One batch over cases [(jpeg, (out_h, out_w), o, ...)] in the library's own buffer -> (pictures, statuses, info)."""
    scale, bias = _constants()
    sc = [_scanned(c[0], flags) for c in cases]
    with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
        b.set_resize([c[1] for c in cases])
        b.set_orientation([c[2] for c in cases])
        if wins is not None:
            b.set_resize_window(wins)
        _filter(b, filt)
        if dtype:
            b.set_normalize(dtype, scale, bias)
        for i, c in enumerate(cases):
            assert b.output_shape(i) == ((3,) + tuple(c[1]) if planar else tuple(c[1]) + (3,))
        b.upload(); b.decode()
        outs, st = b.download()
        return outs, st, b.info()


def _constants():
    from pjd_amd import tensors
    return tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)


def _check(cases, outs, planar, filt, dtype=0):
    scale, bias = _constants()
    for k, (c, o) in enumerate(zip(cases, outs)):
        u8 = c[3][filt]
        want = _layout(nm.normalize(u8, dtype, scale, bias) if dtype else u8, planar)
        assert o.shape == want.shape, (k, c[1], c[2])
        bad = np.argwhere(nm.bits(o) != nm.bits(want)) if dtype else np.argwhere(o != want)
        assert bad.size == 0, (k, "delivered (h, w)", c[1], "orientation", c[2], filt, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 1: every shape in every orientation, one launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_shape_in_every_orientation(ctx, shape_cases, fmt, filt):
    planar = fmt == "planar"
    outs, st, info = _run(ctx, shape_cases, planar, filt)
    assert st == [0] * len(shape_cases)
    assert info["out_bytes"] == sum(3 * h * w for _, (h, w), _, _ in shape_cases)
    _check(shape_cases, outs, planar, filt)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_normalized_output_in_every_orientation(ctx, shape_cases, fmt, filt, dtype):
    """(259, 13) and (8, 8) in the library's own buffer (aligned: the vector stores) for every filter, layout and dtype."""
    planar = fmt == "planar"
    cases = shape_cases[0:8] + shape_cases[16:24]
    assert {c[1] for c in cases} == {(13, 259), (259, 13), (8, 8)}
    outs, st, _ = _run(ctx, cases, planar, filt, dtype)
    assert st == [0] * len(cases)
    _check(cases, outs, planar, filt, dtype)


# ---- 2: bound, unaligned output with guard bands, decoded twice over different pre-fills -------------------------------------------------------
@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_unaligned_output_over_two_prefills(ctx, shape_cases, fmt, filt, dtype):
    """(259, 13), (5, 259) and (8, 8) in all orientations bound into the decoded pictures of two donor batches (two different pre-fills
    of caller-owned memory): uint8 pictures 1, 2 and 3 bytes off a dword, float pictures an odd number of elements off, gaps between
    them as guard bands.  After each decode every picture is the model's and every byte outside the pictures still the donor's."""
    import pjd_amd
    planar = fmt == "planar"
    es = nm.ESIZE[dtype] if dtype else 1
    scale, bias = _constants()
    cases = shape_cases[0:24]
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
            u8 = c[3][filt]
            want = _layout(nm.normalize(u8, dtype, scale, bias) if dtype else u8, planar)
            assert size == want.nbytes and after[off:off + size].tobytes() == want.tobytes(), (c[1], c[2])
            covered[off:off + size] = True
        stray = np.flatnonzero(~covered & (after != pattern))
        assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"
        results.append(pattern[:offs[-1] + sizes[-1]])
    assert not np.array_equal(results[0], results[1]), "the two pre-fills differ"


# ---- 3: windows in Q's coordinates under an orientation ---------------------------------------------------------------------------------------
# Q's target is 30 x 20 (w x h) from the 61 x 45 picture
WINDOWS = [dict(x=3, y=5, w=40, h=30, flags=1), dict(vw=40, vh=40, ox=2, oy=1), dict(x=20, y=10, w=41, h=35, vw=33, vh=27, ox=3, oy=7), dict(vw=40, ox=3)]


@pytest.fixture(scope="module")
def window_cases(sources):
    data, rgb = sources[(61, 45, 53)]
    out, met = [], set()
    for win in WINDOWS:
        for o in ORIS:
            out.append((data, _delivered(30, 20, o), o, {f: _case(rgb, win, 30, 20, o, f, met, (win, o, f)) for f in FILTERS}, win))
    # valid only against the SWAPPED target: delivered 20 x 30 (w x h) in orientation 6, so Q is 30 x 20 and fits the 32 x 21 virtual target
    win = dict(vw=32, vh=21, ox=2, oy=1)
    out.append((data, (30, 20), 6, {f: _case(rgb, win, 30, 20, 6, f, met, (win, 6, f)) for f in FILTERS}, win))
    assert not om._valid(win, 61, 45, 20, 30)
    assert met == {"ignored", "no_mirrors", "exchanged_6_8", "mirrors_first", "unswapped_target"}, met
    return out


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_windows_under_an_orientation(ctx, window_cases, fmt, filt):
    planar = fmt == "planar"
    outs, st, _ = _run(ctx, window_cases, planar, filt, wins=[c[4] for c in window_cases])
    assert st == [0] * len(window_cases)
    _check(window_cases, outs, planar, filt)


def test_a_window_valid_only_against_the_unswapped_target_is_refused(ctx, sources):
    import pjd_amd
    L = pjd_amd.dev_lib()
    data, rgb = sources[(61, 45, 53)]
    win = dict(vw=21, vh=32, ox=1, oy=2)                    # delivered 20 x 30 fits it; Q, 30 x 20, does not
    assert om._valid(win, 61, 45, 20, 30) and not om._valid(win, 61, 45, 30, 20)
    sc = [_scanned(data, 0) for _ in range(2)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(30, 20), (30, 20)])
        b.set_orientation([1, 6])
        arr = (pjd_amd.ResizeWindow * 2)(pjd_amd.ResizeWindow(**win), pjd_amd.ResizeWindow(**win))
        assert L.pjd_batch_set_resize_window(b._h, arr) == E_ARG
        assert b"picture 1" in L.pjd_last_error(ctx._h), L.pjd_last_error(ctx._h)
        b.upload(); b.decode()                              # refused: oriented, without windows
        outs, st = b.download()
    assert st == [0, 0]
    assert np.array_equal(outs[0], om.oriented(rgb, None, 20, 30, 1)) and np.array_equal(outs[1], om.oriented(rgb, None, 20, 30, 6))


# ---- 4: the other paths into the launch -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_pictures(port):
    out = {}
    for n in ("noise_80x96_422_q50_opt", HUFF_ERR[0]):
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    assert out[HUFF_ERR[0]][0] != 0
    return out


@pytest.mark.parametrize("mode", ["scale_1_2", "entropy_error", "sequential", "graph"])
@pytest.mark.parametrize("filt", FILTERS)
def test_other_paths_into_the_launch(ctx, fixture_pictures, filt, mode):
    """PJD_F_SCALE_1_2 in front, a fixture with an entropy-coding error (the partial picture with grey, its status kept), the exact
    kernel (PJD_F_FORCE_SEQUENTIAL), and a captured graph replayed twice: all eight orientations, planar, Q's target 19 x 11."""
    import pjd_amd
    name = HUFF_ERR[0] if mode == "entropy_error" else "noise_80x96_422_q50_opt"
    status, rgb = fixture_pictures[name]
    flags, s = (16, 2) if mode == "scale_1_2" else (pjd_amd.F_FORCE_SEQUENTIAL if mode == "sequential" else 0, 1)
    src = box(rgb, s)
    met = set()
    cases = [(golden_bytes(name), _delivered(19, 11, o), o, {filt: _case(src, None, 19, 11, o, filt, met, (name, o))}) for o in ORIS]
    if mode != "graph":
        outs, st, info = _run(ctx, cases, True, filt, flags=flags)
        if mode == "sequential":
            assert info["n_sequential"] == len(cases)
    else:
        sc = [_scanned(c[0], 0) for c in cases]
        with ctx.batch([x.desc for x in sc], _fmt(True)) as b:
            b.set_resize([c[1] for c in cases])
            b.set_orientation([c[2] for c in cases])
            _filter(b, filt)
            b.upload(); b.capture()
            for _ in range(2):
                b.decode(); b.sync()
            outs, st = b.download()
    assert st == [status] * len(cases)
    _check(cases, outs, True, filt)


# ---- 5: the identity, the records, the launch's name ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_all_ones_equal_a_batch_without_the_call(ctx, fmt, filt):
    import pjd_amd
    names = ["big_640x480_420_q85", "env_61x45_444_q85_opt", "gray_33x70", HUFF_ERR[0]]
    sizes = [(224, 224), (9, 257), (70, 33), (12, 11)]
    res = []
    for call in (False, True):
        sc = [_scanned(golden_bytes(n), 0) for n in names]
        with ctx.batch([x.desc for x in sc], _fmt(fmt == "planar")) as b:
            b.set_resize(sizes)
            if call:
                b.set_orientation([1] * b.n)
            b.set_resize_window([None, dict(x=1, y=2, w=50, h=40, flags=1), None, None])
            _filter(b, filt)
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
            res.append((outs, st, [b.output_size(i) for i in range(b.n)], info["out_bytes"], info["device_bytes"]))
    assert res[0][1:] == res[1][1:] and any(res[0][1])
    for n, a, c in zip(names, res[0][0], res[1][0]):
        assert a.shape == c.shape and np.array_equal(a, c), n


def test_the_records_are_counted_once_and_the_launch_is_named_resize(ctx, sources):
    import pjd_amd
    data, _ = sources[(61, 45, 53)]
    sc = [_scanned(data, 0) for _ in ORIS]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize([_delivered(30, 20, o) for o in ORIS])
        before = b.info()["device_bytes"]
        b.set_orientation(ORIS)
        assert b.info()["device_bytes"] == before + 40 * len(ORIS), "the records are counted"
        b.set_resize_window([dict(x=1, y=1, w=50, h=40)] * len(ORIS))
        assert b.info()["device_bytes"] == before + 40 * len(ORIS), "... and the windows take none of their own"
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize", per
        assert total >= per["resize"]


# ---- 6: call order and arguments ----------------------------------------------------------------------------------------------------------------
def _u8(*v):
    return (C.c_uint8 * len(v))(*v)


def test_set_orientation_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok = _u8(6, 3)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    win = (pjd_amd.ResizeWindow * 2)()
    assert L.pjd_batch_set_orientation(None, ok) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # no resize is set
        b.set_resize(sizes)
        assert L.pjd_batch_set_orientation(b._h, ok) == 0
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # twice
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_orientation(b._h, _u8(1, 1)) == 0
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # twice, the first one all 1
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_window(b._h, win) == 0
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # after set_resize_window
    for filt in (pjd_amd.RESIZE_BILINEAR, pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BICUBIC):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_resize_filter(filt)
            assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                    # after set_resize_filter
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0          # which sets the identity resize itself
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # after upload
        b.decode()
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # after decode
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload(); b.capture()
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # after capture
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                    # after bind_output
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_orientation(b._h, ok) == E_STATE                        # a BMP batch takes no resize, so no orientation
    with pytest.raises(ValueError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_orientation([1])


def test_set_orientation_argument_errors_name_the_picture_and_leave_the_batch_as_it_was(ctx, port):
    import pjd_amd
    import resize_model
    L = pjd_amd.dev_lib()
    names = ["gray_33x70", "env_61x45_420_q100_opt"]
    rgb = [port.decode(golden_bytes(n))["rgb"] for n in names]
    sc = [_scanned(golden_bytes(n), 0) for n in names]
    sizes = [(31, 17), (20, 30)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        assert L.pjd_batch_set_orientation(b._h, None) == E_ARG                        # a null array changes nothing
        for bad in (0, 9, 255):
            assert L.pjd_batch_set_orientation(b._h, _u8(6, bad)) == E_ARG, bad
            assert b"picture 1" in L.pjd_last_error(ctx._h), (bad, L.pjd_last_error(ctx._h))
        assert L.pjd_batch_set_orientation(b._h, _u8(0, 6)) == E_ARG
        assert b"picture 0" in L.pjd_last_error(ctx._h)
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                         # after the refused calls: unoriented
        outs, st = b.download()
    assert st == [0, 0]
    for p, (th, tw), o in zip(rgb, sizes, outs):
        assert np.array_equal(o, resize_model.resize(p, tw, th))
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:                       # ... and the call is still open after a refusal
        b.set_resize(sizes)
        assert L.pjd_batch_set_orientation(b._h, _u8(9, 1)) == E_ARG
        b.set_orientation([8, 3])
        b.upload(); b.decode()
        outs, st = b.download()
    for p, (th, tw), o, ori in zip(rgb, sizes, outs, (8, 3)):
        assert np.array_equal(o, om.oriented(p, None, tw, th, ori)), ori


# ---- 7: the torch side, in a child process (tests/orientation_torch_cases.py imports torch first) ---------------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "orientation_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_tensor_helpers_with_orientations_equal_the_model():
    """decode_to_tensors, decode_resized_batch_tensor (crops of the upright picture, flips, three filters) and
    decode_normalized_batch_tensor (resize_short, channels_last bf16) with orientations= against the model."""
    _torch_case("orientations_against_the_model")


def test_tensor_helpers_are_within_one_level_of_torch_orient_crop_interpolate():
    _torch_case("within_one_level_of_orient_crop_interpolate")
