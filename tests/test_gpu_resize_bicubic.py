"""The bicubic resize on decode (pjd_batch_set_resize_filter, PJD_RESIZE_BICUBIC) on the GPU (run with -m gpu on an MI355X).  Every
expectation is tests/resize_bicubic_model.py -- the numpy model of the arithmetic include/pjd.h specifies -- over the box filter of
the oracle's picture (through crop -> model -> crop -> flip for a source window), transposed for planar, and every comparison is byte
(bit, for floats) equality; never something this library resized.  Geometry and fixtures are those of tests/test_gpu_resize_aa.py
and tests/test_gpu_resize_window.py.  Every refusal asked for here is a return code of the host side."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import resize_bicubic_model as bc
import resize_window_model as wm
from conftest import golden_bytes
from test_gpu_resize import HUFF_ERR, MANIFEST, SCALES, VALID, _scanned
from test_gpu_resize_aa import BOUND, DT_NAME, DTYPES, GEOMETRY, _fmt, _synth, target_of
from test_gpu_resize_window import GEOMETRY as WINDOWS
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5


def _layout(pic, planar):
    return np.ascontiguousarray(pic.transpose(2, 0, 1)) if planar else pic


def windowed(rgb, win, tw, th):
    """flip(model(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]) of include/pjd.h, with the bicubic model."""
    P = np.asarray(rgb)
    r = wm.resolve(win, P.shape[1], P.shape[0], tw, th)
    v = bc.resize(P[r["y"]:r["y"] + r["h"], r["x"]:r["x"] + r["w"]], r["vw"], r["vh"])
    out = v[r["oy"]:r["oy"] + th, r["ox"]:r["ox"] + tw]
    return np.ascontiguousarray(out[:, ::-1] if r["flags"] & wm.HFLIP else out)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(port):
    out = {}
    for n in VALID:
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    return out


@pytest.fixture(scope="module")
def fixture_cases(oracle):
    """The cases of the all-fixtures batch, the interleaved expectation of each computed once:
    [(fixture, scale flags, (th, tw), status, th x tw x 3 picture)] -- pre-scales round-robin, the targets of target_of."""
    out = []
    for k, n in enumerate(VALID):
        flags, s = SCALES[k % 4]
        sw, sh = -(-MANIFEST[n]["dims"][0] // s), -(-MANIFEST[n]["dims"][1] // s)
        tw, th = target_of(k // 4 + k % 4, sw, sh)
        out.append((n, flags, (th, tw), oracle[n][0], bc.resize(box(oracle[n][1], s), tw, th)))
    assert any(st != 0 for _, _, _, st, _ in out), "an entropy error is among them"
    return out


# ---- 1: every fixture in one batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_fixture_bicubic_in_one_batch(ctx, fixture_cases, mode, fmt):
    import pjd_amd
    planar = fmt == "planar"
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    scanned = [_scanned(golden_bytes(n), flags | extra) for n, flags, _, _, _ in fixture_cases]
    sizes = [t for _, _, t, _, _ in fixture_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        assert b.info()["device_bytes"] > before, "the weight table is counted"
        for i, (th, tw) in enumerate(sizes):
            assert b.output_size(i) == 3 * tw * th and b.output_shape(i) == ((3, th, tw) if planar else (th, tw, 3))
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    if mode == "exact":
        assert info["n_sequential"] == len(scanned)
    assert info["out_bytes"] == sum(3 * tw * th for th, tw in sizes)
    for (n, flags, (th, tw), status, want), o, got_st in zip(fixture_cases, outs, st):
        want = _layout(want, planar)
        assert got_st == status, (n, flags)
        assert o.shape == want.shape and np.array_equal(o, want), (n, flags, tw, th, int(np.abs(o.astype(int) - want).max()))


# ---- 2: entropy-coding errors -----------------------------------------------------------------------------------------------------
def test_entropy_error_fixtures_keep_status_and_resize_the_partial_picture(ctx, oracle):
    import pjd_amd
    assert HUFF_ERR
    scanned, sizes, want = [], [], []
    for k, n in enumerate(HUFF_ERR):
        flags, s = SCALES[k % 4]
        sc = _scanned(golden_bytes(n), flags)
        sw, sh = pjd_amd.scaled_dims(sc.desc.width, sc.desc.height, flags)
        tw, th = target_of(k + 1, sw, sh) if k % 3 else (max(sw // 3, 1), max(sh // 2, 1))
        scanned.append(sc); sizes.append((th, tw)); want.append((n, oracle[n][0], bc.resize(box(oracle[n][1], s), tw, th)))
    with ctx.batch([x.desc for x in scanned], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.upload(); b.decode()
        outs, st = b.download()
    for (n, status, pic), o, got_st in zip(want, outs, st):
        assert got_st == status != 0, n
        assert np.array_equal(o, pic), n


# ---- 3: geometry the tiling can get wrong, the tap limit, an upscale, the identity ---------------------------------------------------------
# GEOMETRY of the antialiased tests (a tile crossed with a ragged last lane group, 33 row tiles, 64 -> 4: 16x on both axes with every
# support clipped by the picture, a second tile of one column, an upscale) and: the axis that attains 64 taps at i = 3; the same size, which must be the
# picture itself; both at once on one axis each
MORE = [((96, 40, 91), (6, 5)),
        ((61, 45, 92), (61, 45)),
        ((96, 23, 93), (6, 23))]


@pytest.fixture(scope="module")
def geometry_cases(port):
    synth = _synth()
    out = []
    for (w, h, seed), (tw, th) in GEOMETRY + MORE:
        data = synth.make(w, h, seed, 90, synth.SUB_444)
        rgb = port.decode(data)["rgb"]
        want = bc.resize(rgb, tw, th)
        if (tw, th) == (w, h):
            assert np.array_equal(want, rgb), "the same size reproduces the picture"
        out.append((data, (th, tw), want))
    assert int(bc.axis_taps(96, 6)[1].max()) == bc.MAX_TAPS    # 64 -> 4 is 16x too, but the picture's edges clip every support there
    return out


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_tile_edges_the_tap_limit_an_upscale_and_the_identity(ctx, geometry_cases, fmt):
    import pjd_amd
    planar = fmt == "planar"
    scanned = [_scanned(data, 0) for data, _, _ in geometry_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, t, _ in geometry_cases])
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0] * len(geometry_cases)
    for (_, (th, tw), want), o in zip(geometry_cases, outs):
        want = _layout(want, planar)
        bad = np.argwhere(o != want)
        assert o.shape == want.shape and bad.size == 0, (tw, th, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 4: a 0/255 checkerboard: the one clamp at both ends ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker_case(port):
    """A 64 x 48 JPEG of 8 x 8 cells of 0 and 255 (every block flat: it decodes to the extremes), shrunk along x and grown along y:
    the model's value before the clamp leaves 0..255 on both sides, so a kernel that clamped between the passes, or not at all,
    or wrapped, gives other bytes."""
    from PIL import Image
    yy, xx = np.mgrid[0:48, 0:64]
    cells = ((((xx >> 3) + (yy >> 3)) & 1) * 255).astype(np.uint8)
    bio = io.BytesIO()
    Image.fromarray(np.repeat(cells[:, :, None], 3, axis=2), "RGB").save(bio, "JPEG", quality=100, subsampling=0)
    data = bio.getvalue()
    rgb = port.decode(data)["rgb"]
    assert rgb.min() <= 2 and rgb.max() >= 253
    stats = {}
    want = bc.resize(rgb, 45, 70, stats)
    assert stats["below"] > 0 and stats["above"] > 0 and want.min() == 0 and want.max() == 255
    hz = bc.horizontal_f64(rgb, 45)
    assert hz.min() < -1 and hz.max() > 256, "the horizontal pass alone overshoots: a clamp between the passes would show"
    return data, (70, 45), want


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_checkerboard_clamps_at_both_ends(ctx, checker_case, fmt):
    import pjd_amd
    data, size, want = checker_case
    sc = _scanned(data, 0)
    with ctx.batch([sc.desc], _fmt(fmt == "planar")) as b:
        b.set_resize([size])
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.upload(); b.decode()
        (o,), st = b.download()
    assert st == [0]
    assert np.array_equal(o, _layout(want, fmt == "planar"))


# ---- 5: source windows ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_cases(port):
    """The geometry of tests/test_gpu_resize_window.py: crops at each dword remainder of x, mirrored and not, on a tile-crossing width;
    a 16x window inside a picture (56 taps an axis, nothing beyond it may contribute); a virtual target with an offset, mirrored too; the
    window's edge where the picture continues; 33 row tiles of a planar source lower than its picture; a 1 x 1 window."""
    synth = _synth()
    decoded, out = {}, []
    for pic, win, (tw, th) in WINDOWS:
        if pic not in decoded:
            data = golden_bytes(pic) if isinstance(pic, str) else synth.make(pic[0], pic[1], pic[2], 90, synth.SUB_444)
            decoded[pic] = (data, port.decode(data)["rgb"])
        data, rgb = decoded[pic]
        want = windowed(rgb, win, tw, th)
        if any(win.get(k, 0) for k in wm.FIELDS):
            assert not np.array_equal(want, bc.resize(rgb, tw, th)), "the window matters"
        if win.get("flags", 0) and win.get("w", 2) > 1:
            assert not np.array_equal(want, want[:, ::-1]), "the mirror matters"
        out.append((data, win, (th, tw), want))
    assert {w.get("x", 0) % 4 for _, w, _, _ in out} == {0, 1, 2, 3} and any(w.get("ox", 0) for _, w, _, _ in out)
    return out


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_window_geometry(ctx, window_cases, fmt):
    import pjd_amd
    planar = fmt == "planar"
    scanned = [_scanned(data, 0) for data, _, _, _ in window_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, _, t, _ in window_cases])
        b.set_resize_window([w for _, w, _, _ in window_cases])
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0] * len(window_cases)
    for k, ((_, win, (th, tw), want), o) in enumerate(zip(window_cases, outs)):
        want = _layout(want, planar)
        bad = np.argwhere(o != want)
        assert o.shape == want.shape and bad.size == 0, (k, win, tw, th, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 6: normalised output; bound, unaligned output on a captured graph ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_normalized_output_is_the_normalize_model_over_the_bicubic_model(ctx, fixture_cases, fmt, dtype):
    """Every fifth fixture case (all four targets, the pre-scales) in the library's own buffer: aligned vector stores."""
    import pjd_amd
    from pjd_amd import tensors
    planar = fmt == "planar"
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    cases = fixture_cases[::5]
    scanned = [_scanned(golden_bytes(n), flags) for n, flags, _, _, _ in cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, _, t, _, _ in cases])
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.set_normalize(dtype, scale, bias)
        b.upload(); b.decode()
        outs, st = b.download()
    for (n, flags, (th, tw), status, u8), o, got_st in zip(cases, outs, st):
        want = _layout(nm.normalize(u8, dtype, scale, bias), planar)
        assert got_st == status, n
        assert o.shape == want.shape and o.dtype == want.dtype and np.array_equal(nm.bits(o), nm.bits(want)), (n, flags, tw, th)


@pytest.fixture(scope="module")
def bound_cases(oracle):
    return [(n, t, oracle[n][0], bc.resize(oracle[n][1], t[1], t[0])) for n, t in BOUND]


@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_unaligned_output_on_a_captured_graph(ctx, bound_cases, fmt, dtype):
    """As the antialiased test of this name: pictures bound into a donor batch's decoded picture, uint8 pictures 1, 2 and 3 bytes off
    a dword, float pictures an odd number of elements off; captured, replayed three times; every picture is the model's and every
    byte outside the pictures still the donor's."""
    import pjd_amd
    from pjd_amd import tensors
    planar = fmt == "planar"
    es = nm.ESIZE[dtype] if dtype else 1
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        donor.upload(); donor.decode()
        (pattern,), _ = donor.download()
        pattern = pattern.reshape(-1).copy()
        mem, cap = donor.device_output(0), donor.output_size(0)
        sc = [_scanned(golden_bytes(n), 0) for n, _, _, _ in bound_cases]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize([t for _, t, _, _ in bound_cases])
            b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
            if dtype:
                b.set_normalize(dtype, scale, bias)
            offs, pos = [], es
            for i in range(b.n):
                while (pos // es) % 4 != (i % 3) + 1:          # 1, 2, 3 elements past a multiple of four elements
                    pos += es
                offs.append(pos)
                pos += b.output_size(i)
            assert pos <= cap and sorted({(o // es) % 4 for o in offs}) == [1, 2, 3]
            b.bind_output(mem, cap, offs)
            b.upload(); b.capture()
            for _ in range(3):
                b.decode(); b.sync()
            outs, st = b.download()
            sizes = [b.output_size(i) for i in range(b.n)]
        (after,), _ = donor.download()
        after = after.reshape(-1)
    covered = np.zeros(cap, bool)
    for (n, (th, tw), status, u8), o, off, size, got_st in zip(bound_cases, outs, offs, sizes, st):
        want = _layout(nm.normalize(u8, dtype, scale, bias) if dtype else u8, planar)
        assert got_st == status and size == want.nbytes, n
        assert o.shape == want.shape and o.tobytes() == want.tobytes(), (n, fmt, DT_NAME[dtype])
        assert after[off:off + size].tobytes() == want.tobytes(), n
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"


# ---- 7: refusals and call order -----------------------------------------------------------------------------------------------------------
def test_a_picture_past_16x_is_refused_and_named(ctx):
    """65 x 64 -> 4 x 4 is past the limit along x (64 x 65 along y): PJD_E_ARG, the picture named, and the batch is left as it was,
    bilinear.  A window past 16x its virtual target is named likewise; behind the 1/2 pre-scale the picture is inside."""
    import pjd_amd
    synth = _synth()
    L = pjd_amd.dev_lib()
    BC = pjd_amd.RESIZE_BICUBIC
    ok = _scanned(synth.make(64, 64, 73, 90, synth.SUB_444), 0)
    for w, h in ((65, 64), (64, 65)):
        bad = _scanned(synth.make(w, h, 76, 90, synth.SUB_444), 0)
        with ctx.batch([ok.desc, bad.desc, ok.desc], pjd_amd.OUT_RGB8) as b:
            b.set_resize([(4, 4)] * 3)
            assert L.pjd_batch_set_resize_filter(b._h, BC) == E_ARG
            assert b"picture 1" in L.pjd_last_error(ctx._h) and b"16x" in L.pjd_last_error(ctx._h)
            with ctx.batch([ok.desc, bad.desc, ok.desc], pjd_amd.OUT_RGB8) as plain:
                plain.set_resize([(4, 4)] * 3)
                plain.upload(); plain.decode()
                want, _ = plain.download()
            b.upload(); b.decode()
            outs, st = b.download()
            assert st == [0, 0, 0] and all(np.array_equal(o, p) for o, p in zip(outs, want))
    bad = _scanned(synth.make(65, 64, 76, 90, synth.SUB_444), 0)
    with ctx.batch([ok.desc, ok.desc, bad.desc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(4, 4)] * 3)
        b.set_resize_window([None, None, (0, 0, 65, 64, 8, 8)])             # inside 16x of the 8 x 8 virtual target
        b.set_resize_filter(BC)
    with ctx.batch([ok.desc, ok.desc, bad.desc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(4, 4)] * 3)
        b.set_resize_window([None, (0, 0, 64, 64), (0, 0, 65, 64)])
        assert L.pjd_batch_set_resize_filter(b._h, BC) == E_ARG
        assert b"picture 2" in L.pjd_last_error(ctx._h) and b"16x" in L.pjd_last_error(ctx._h)
    half = _scanned(synth.make(65, 64, 76, 90, synth.SUB_444), pjd_amd.F_SCALE_1_2)
    with ctx.batch([half.desc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(4, 4)])
        b.set_resize_filter(BC)


def test_set_resize_filter_state_and_argument_errors(ctx):
    import ctypes as C
    import pjd_amd
    L = pjd_amd.dev_lib()
    BC, AA, BL = pjd_amd.RESIZE_BICUBIC, pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BILINEAR
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.pjd_batch_set_resize_filter(None, BC) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize_filter(b._h, BC) == E_STATE                     # before set_resize
        b.set_resize(sizes)
        for bad in (2, 4, -1, 255):
            assert L.pjd_batch_set_resize_filter(b._h, bad) == E_ARG                  # an unknown filter
            assert b"unknown filter" in L.pjd_last_error(ctx._h) and b"PJD_RESIZE_BICUBIC" in L.pjd_last_error(ctx._h)
        assert L.pjd_batch_set_resize_filter(b._h, BC) == 0
        for again in (BC, AA, BL):
            assert L.pjd_batch_set_resize_filter(b._h, again) == E_STATE              # twice
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_filter(b._h, AA) == 0
        assert L.pjd_batch_set_resize_filter(b._h, BC) == E_STATE                     # twice, the first one antialiased
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_resize_filter(b._h, BC) == E_STATE                     # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_resize_filter(b._h, BC) == E_STATE                     # after upload
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_resize_filter(b._h, BC) == E_STATE                 # after bind_output
    with pytest.raises(pjd_amd.PjdError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize_filter(BC)


# ---- 8: timings ---------------------------------------------------------------------------------------------------------------------------
def test_decode_timed_names_the_launch_resize(ctx):
    import pjd_amd
    sc = [_scanned(golden_bytes(n), f) for n, f in (("big_640x480_420_q85", 16), ("ilsvrc_val_00000001", 0), ("gray_61x45", pjd_amd.F_FORCE_SEQUENTIAL))]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize([(224, 224)] * 3)
        b.set_resize_filter(pjd_amd.RESIZE_BICUBIC)
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize", per
        assert total >= per["resize"]


# ---- 9: the torch side, in a child process (tests/resize_bicubic_torch_cases.py imports torch first) ---------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "resize_bicubic_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_decode_resized_batch_tensor_bicubic():
    """16 synthetic pictures of different sizes -> ONE uint8[16, 3, 224, 224] torch tensor equal to the model, with the pre-scale and
    without it, and within 1 level of torch's own bicubic antialias=True on the float picture."""
    _torch_case("resized_batch_tensor")


def test_decode_normalized_batch_tensor_bicubic_channels_last():
    _torch_case("normalized_channels_last")
