"""Source windows of the resize on decode (pjd_batch_set_resize_window) on the GPU (run with -m gpu on an MI355X).  Every expectation
is tests/resize_window_model.py -- crop -> model -> crop -> flip over the two numpy models of include/pjd.h's arithmetic -- over the
box filter of the oracle's picture, and every comparison is byte (bit, for floats) equality; never something this library resized.
The fixtures assert on the CPU, before anything runs on the device, that no expectation is also what a wrong implementation (no
window, taps clamped to the picture, flip ignored, offset ignored) would deliver."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import resize_window_model as wm
from conftest import golden_bytes, ROOT
from test_gpu_resize import HUFF_ERR, MANIFEST, SCALES, VALID, _scanned
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
FILTERS = ["bilinear", "antialias"]


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


def _layout(pic, planar):
    return np.ascontiguousarray(pic.transpose(2, 0, 1)) if planar else pic


def _set(b, sizes, wins, antialias):
    import pjd_amd
    b.set_resize(sizes)
    b.set_resize_window(wins)
    if antialias:
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)


def _not_a_wrong_model(rgb, win, tw, th, antialias, want, what):
    """A vacuous case is a test bug: the expectation must differ from every wrong model that applies to the case."""
    wrong = wm.wrong_models(rgb, win, tw, th, antialias)
    for name, pic in wrong.items():
        assert pic.shape == want.shape and not np.array_equal(pic, want), (what, "the expectation is also that of the wrong model", name)
    return set(wrong)


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


# ---- 1: geometry the windows can get wrong ------------------------------------------------------------------------------------------------
def W(x=0, y=0, w=0, h=0, vw=0, vh=0, ox=0, oy=0, flip=False):
    return {k: v for k, v in dict(x=x, y=y, w=w, h=h, vw=vw, vh=vh, ox=ox, oy=oy, flags=wm.HFLIP if flip else 0).items() if v}


# (picture: (w, h, seed) of a synthetic one or a fixture's name, window, (tw, th))
GEOMETRY = (
    # all four dword remainders of the staged segment's first byte, in both layouts (planar: x + xs, interleaved: 3 * (x + xs)); 259 columns
    # cross the 256-column tile edge and leave a ragged last lane group; mirrored and not.  (x = 4 takes w = 596: 4 + 597 is past 600)
    [((600, 40, 81), W(x, 2, 597 if x < 4 else 596, 35, flip=f), (259, 5)) for x in (1, 2, 3, 4) for f in (False, True)] + [
    # 32 taps on both axes inside an interior window: nothing beyond it may contribute
    ((200, 120, 82), W(100, 40, 64, 64), (4, 4)),
    # the whole picture (a zero window) to a virtual target larger than what is delivered; the offset crosses a tile; growing
    ((300, 20, 83), W(vw=600, vh=20, ox=250, oy=3), (270, 9)),
    ((300, 20, 83), W(vw=600, vh=20, ox=250, oy=3, flip=True), (270, 9)),
    # the clamp at the window's edge where the picture continues (right and below), and where picture and window end together
    ((61, 45, 84), W(0, 0, 21, 15), (50, 33)),
    ((61, 45, 84), W(40, 30, 21, 15), (50, 33)),
    # 33 row tiles with taps beyond their own rows; the plane stride of a planar source with h != sh
    ((40, 600, 85), W(3, 7, 30, 580, flip=True), (5, 259)),
    # a 1 x 1 window: constant output
    ("gray_33x70", W(5, 9, 1, 1, flip=True), (9, 7))])


@pytest.fixture(scope="module")
def geometry_cases(port):
    """[(jpeg bytes, window, (th, tw), {filter: th x tw x 3 expectation})]; every wrong model is met by some case of each filter."""
    synth = _synth()
    decoded, out = {}, []
    met = {f: set() for f in FILTERS}
    for pic, win, (tw, th) in GEOMETRY:
        if pic not in decoded:
            data = golden_bytes(pic) if isinstance(pic, str) else synth.make(pic[0], pic[1], pic[2], 90, synth.SUB_444)
            decoded[pic] = (data, port.decode(data)["rgb"])
        data, rgb = decoded[pic]
        want = {}
        for f in FILTERS:
            want[f] = wm.window(rgb, win, tw, th, f == "antialias")
            met[f] |= _not_a_wrong_model(rgb, win, tw, th, f == "antialias", want[f], (pic, win, f))
        out.append((data, win, (th, tw), want))
    one = out[-1][3]
    assert all((one[f] == one[f][0, 0]).all() for f in FILTERS), "a 1 x 1 window gives a constant picture"
    assert all(met[f] == {"no_window", "picture_clamp", "no_flip", "no_offset"} for f in FILTERS), met
    return out


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_window_geometry(ctx, geometry_cases, fmt, filt):
    planar = fmt == "planar"
    scanned = [_scanned(data, 0) for data, _, _, _ in geometry_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, _, t, _ in geometry_cases])
        before = b.info()["device_bytes"]
        b.set_resize_window([w for _, w, _, _ in geometry_cases])
        assert b.info()["device_bytes"] == before + 40 * len(geometry_cases), "the records are counted"
        if filt == "antialias":
            import pjd_amd
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0] * len(geometry_cases)
    for k, ((_, win, (th, tw), want), o) in enumerate(zip(geometry_cases, outs)):
        want = _layout(want[filt], planar)
        bad = np.argwhere(o != want)
        assert o.shape == want.shape and bad.size == 0, (k, win, tw, th, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 2: all-zero records are the identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_zero_records_equal_a_batch_without_the_call(ctx, fmt, filt):
    import pjd_amd
    names = ["big_640x480_420_q85", "env_61x45_444_q85_opt", "gray_33x70", "wrap_420_q65535"] + HUFF_ERR[:1]
    sizes = [(224, 224), (9, 257), (70, 33), (5, 7), (12, 11)]
    res = []
    for call in (False, True):
        sc = [_scanned(golden_bytes(n), SCALES[k % 2][0]) for k, n in enumerate(names)]
        with ctx.batch([x.desc for x in sc], _fmt(fmt == "planar")) as b:
            b.set_resize(sizes)
            if call:
                b.set_resize_window([None] * b.n)
            if filt == "antialias":
                b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
            res.append((outs, st, [b.output_size(i) for i in range(b.n)], info["out_bytes"], info["device_bytes"]))
    assert res[0][1:] == res[1][1:] and any(res[0][1])
    for n, a, c in zip(names, res[0][0], res[1][0]):
        assert a.shape == c.shape and np.array_equal(a, c), n


# ---- 3: every fixture in one batch ------------------------------------------------------------------------------------------------------------
def seeded_window(rng, sw, sh, flip):
    """A window, a virtual target and a delivered part for a picture of sw x sh at its decode size, inside the antialiased filter's 16x
    limit: (window dict, (th, tw))."""
    w, h = int(rng.integers(max(1, sw // 4), sw + 1)), int(rng.integers(max(1, sh // 4), sh + 1))
    x, y = int(rng.integers(0, sw - w + 1)), int(rng.integers(0, sh - h + 1))
    tw, th = [(7, 5), (33, 17), (64, 64), (w, h), (2 * w + 3, h // 2 + 1)][int(rng.integers(0, 5))]
    vw, vh = tw + int(rng.integers(0, 3)) * 5, th + int(rng.integers(0, 2)) * 3
    vw, vh = max(vw, -(-w // 16)), max(vh, -(-h // 16))
    ox, oy = int(rng.integers(0, vw - tw + 1)), int(rng.integers(0, vh - th + 1))
    return W(x, y, w, h, vw, vh, ox, oy, flip), (th, tw)


@pytest.fixture(scope="module")
def fixture_cases(oracle):
    """[(fixture, scale flags, window, (th, tw), status, {filter: expectation})]: pre-scales round-robin, seeded windows, every second
    picture mirrored."""
    rng = np.random.default_rng(20)
    out = []
    for k, n in enumerate(VALID):
        flags, s = SCALES[k % 4]
        src = box(oracle[n][1], s)
        sh, sw = src.shape[:2]
        assert (sw, sh) == (-(-MANIFEST[n]["dims"][0] // s), -(-MANIFEST[n]["dims"][1] // s))
        win, (th, tw) = seeded_window(rng, sw, sh, k % 2 == 1)
        want = {f: wm.window(src, win, tw, th, f == "antialias") for f in FILTERS}
        out.append((n, flags, win, (th, tw), oracle[n][0], want))
    assert HUFF_ERR and all(st != 0 for n, _, _, _, st, _ in out if n in HUFF_ERR)
    return out


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_fixture_windowed_in_one_batch(ctx, fixture_cases, fmt, filt, mode):
    """All decodable fixtures (the entropy-error ones among them: their status stays and the windowed PARTIAL picture matches), on the
    parallel decoder and on the exact kernel."""
    import pjd_amd
    planar = fmt == "planar"
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    scanned = [_scanned(golden_bytes(n), flags | extra) for n, flags, _, _, _, _ in fixture_cases]
    sizes = [t for _, _, _, t, _, _ in fixture_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        _set(b, sizes, [w for _, _, w, _, _, _ in fixture_cases], filt == "antialias")
        for i, (th, tw) in enumerate(sizes):
            assert b.output_size(i) == 3 * tw * th and b.output_shape(i) == ((3, th, tw) if planar else (th, tw, 3))
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    if mode == "exact":
        assert info["n_sequential"] == len(scanned)
    assert info["out_bytes"] == sum(3 * tw * th for th, tw in sizes)
    for (n, flags, win, (th, tw), status, want), o, got_st in zip(fixture_cases, outs, st):
        want = _layout(want[filt], planar)
        assert got_st == status, (n, flags)
        assert o.shape == want.shape and np.array_equal(o, want), (n, flags, win, tw, th, int(np.abs(o.astype(int) - want).max()))


# ---- 4: bound, unaligned output on a captured graph; normalised output ------------------------------------------------------------------
# (fixture, window, (th, tw)): tw of 257, 259, 61, 7, 224
BOUND = [("wrap_420_q65535", W(vw=300, vh=12, ox=40, oy=2, flip=True), (9, 257)),
         ("big_640x480_420_q85", W(13, 7, 518, 40, flip=True), (5, 259)),
         ("env_61x45_444_q85_opt", W(vw=70, vh=45, ox=9), (45, 61)),
         ("noise_80x96_422_q50_opt", W(3, 5, 70, 90), (17, 7)),
         ("big_640x480_420_q85", W(101, 50, 400, 380, flip=True), (224, 224))]


@pytest.fixture(scope="module")
def bound_cases(oracle):
    out = []
    for n, win, (th, tw) in BOUND:
        want = {f: wm.window(oracle[n][1], win, tw, th, f == "antialias") for f in FILTERS}
        for f in FILTERS:
            _not_a_wrong_model(oracle[n][1], win, tw, th, f == "antialias", want[f], (n, win, f))
        out.append((n, win, (th, tw), oracle[n][0], want))
    return out


@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_unaligned_output_on_a_captured_graph(ctx, bound_cases, fmt, filt, dtype):
    """Five windowed pictures, three of them mirrored, bound into device memory that holds a known pattern (a donor batch's decoded
    picture), uint8 pictures 1, 2 and 3 bytes off a dword, float pictures an odd number of elements off.  The decode is captured and
    replayed three times; then every picture is the model's (normalised by tests/normalize_model.py, bit for bit) and every byte
    outside the pictures still the donor's."""
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
        assert mem % 256 == 0
        sc = [_scanned(golden_bytes(n), 0) for n, _, _, _, _ in bound_cases]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            _set(b, [t for _, _, t, _, _ in bound_cases], [w for _, w, _, _, _ in bound_cases], filt == "antialias")
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
    for (n, win, (th, tw), status, u8), o, off, size, got_st in zip(bound_cases, outs, offs, sizes, st):
        want = nm.normalize(u8[filt], dtype, scale, bias) if dtype else u8[filt]
        want = _layout(want, planar)
        assert got_st == status and size == want.nbytes, n
        assert o.shape == want.shape and o.tobytes() == want.tobytes(), (n, win, fmt, filt, DT_NAME[dtype])
        assert after[off:off + size].tobytes() == want.tobytes(), n
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_normalized_output_is_the_normalize_model_over_the_window_model(ctx, fixture_cases, fmt, filt, dtype):
    """Every fifth fixture case in the library's own buffer: aligned vector stores, where the bound test has element stores."""
    import pjd_amd
    from pjd_amd import tensors
    planar = fmt == "planar"
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    cases = fixture_cases[::5]
    assert len({f for _, f, _, _, _, _ in cases}) == 4 and any(w.get("flags") for _, _, w, _, _, _ in cases)
    scanned = [_scanned(golden_bytes(n), flags) for n, flags, _, _, _, _ in cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        _set(b, [t for _, _, _, t, _, _ in cases], [w for _, _, w, _, _, _ in cases], filt == "antialias")
        b.set_normalize(dtype, scale, bias)
        b.upload(); b.decode()
        outs, st = b.download()
    for (n, flags, win, (th, tw), status, u8), o, got_st in zip(cases, outs, st):
        want = _layout(nm.normalize(u8[filt], dtype, scale, bias), planar)
        assert got_st == status, n
        assert o.shape == want.shape and o.dtype == want.dtype and np.array_equal(nm.bits(o), nm.bits(want)), (n, flags, win, tw, th)


# ---- 5: call order and arguments ------------------------------------------------------------------------------------------------------------
def _recs(*wins):
    import pjd_amd
    arr = (pjd_amd.ResizeWindow * len(wins))()
    for i, w in enumerate(wins):
        arr[i] = pjd_amd.ResizeWindow(**w)
    return arr


def test_set_resize_window_state_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    AA = pjd_amd.RESIZE_ANTIALIAS
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    ok = _recs(dict(x=1, y=1, w=40, h=30), {})
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.pjd_batch_set_resize_window(None, ok) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # before set_resize
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_window(b._h, None) == E_ARG                     # a null array changes nothing
        assert L.pjd_batch_set_resize_window(b._h, ok) == 0
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # twice
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_window(b._h, _recs({}, {})) == 0
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # twice, the first one all zero
    for filt in (pjd_amd.RESIZE_BILINEAR, AA):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_resize_filter(filt)
            assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                 # after set_resize_filter
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0         # which sets the identity resize itself
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # after upload
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                 # after bind_output
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        w, h = (C.c_uint32 * 2)(30, 17), (C.c_uint32 * 2)(20, 31)
        assert L.pjd_batch_set_resize(b._h, w, h) == E_ARG                            # a BMP batch is never resized ...
        assert L.pjd_batch_set_resize_window(b._h, ok) == E_STATE                     # ... so it has no window to take
    with pytest.raises(pjd_amd.PjdError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize_window([None, None])
    with pytest.raises(ValueError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.set_resize_window([None])


# every rule of include/pjd.h for a 61 x 45 picture with the target 30 x 20 (w x h)
BAD_WINDOWS = [dict(h=10), dict(w=10), dict(x=1), dict(y=1), dict(x=41, y=0, w=21, h=15), dict(x=0, y=31, w=21, h=15), dict(vw=65536),
               dict(vh=65536), dict(vw=40, ox=11), dict(vh=30, oy=11), dict(ox=1), dict(oy=1), dict(flags=2), dict(reserved_=1)]


def test_set_resize_window_argument_errors_name_the_picture_and_leave_the_batch_unwindowed(ctx, oracle):
    import pjd_amd
    import resize_model
    L = pjd_amd.dev_lib()
    names = ["gray_33x70", "env_61x45_420_q100_opt"]
    sc = [_scanned(golden_bytes(n), 0) for n in names]
    sizes = [(31, 17), (20, 30)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        for bad in BAD_WINDOWS:
            assert pjd_amd.resize_window_check(61, 45, 30, 20, bad) is False, bad
            assert L.pjd_batch_set_resize_window(b._h, _recs(dict(x=2, y=3, w=20, h=40), bad)) == E_ARG, bad
            assert b"picture 1" in L.pjd_last_error(ctx._h), (bad, L.pjd_last_error(ctx._h))
        assert L.pjd_batch_set_resize_window(b._h, _recs(dict(x=14, y=0, w=20, h=40), {})) == E_ARG
        assert b"picture 0" in L.pjd_last_error(ctx._h)
        assert b.info()["device_bytes"] == before
        b.upload(); b.decode()                                                        # after the refused calls: un-windowed
        outs, st = b.download()
    assert st == [0, 0]
    for n, (th, tw), o in zip(names, sizes, outs):
        assert np.array_equal(o, resize_model.resize(oracle[n][1], tw, th)), n


def test_the_16x_limit_is_the_windows(ctx, port):
    """200 x 120 -> 4 x 4 is past the antialiased filter's limit as a whole picture; with the window (100, 40, 64, 64) it is inside and
    accepted, with (100, 40, 65, 64) refused and named -- by set_resize_filter, which is where the filter is known."""
    import pjd_amd
    synth = _synth()
    L = pjd_amd.dev_lib()
    data = synth.make(200, 120, 82, 90, synth.SUB_444)
    small = synth.make(64, 64, 73, 90, synth.SUB_444)
    rgb = port.decode(data)["rgb"]
    for win, rc in ((dict(x=100, y=40, w=64, h=64), 0), (dict(x=100, y=40, w=65, h=64), E_ARG), (dict(x=100, y=40, w=64, h=65), E_ARG), ({}, E_ARG)):
        sc = [_scanned(small, 0), _scanned(data, 0)]
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
            b.set_resize([(4, 4)] * 2)
            assert L.pjd_batch_set_resize_window(b._h, _recs(dict(flags=1), win)) == 0        # the bilinear filter has no such limit
            assert L.pjd_batch_set_resize_filter(b._h, pjd_amd.RESIZE_ANTIALIAS) == rc, win
            if rc:
                assert b"picture 1" in L.pjd_last_error(ctx._h) and b"16x" in L.pjd_last_error(ctx._h)
            b.upload(); b.decode()                          # refused: the batch stays bilinear, and windowed
            outs, st = b.download()
        assert st == [0, 0]
        assert np.array_equal(outs[1], wm.window(rgb, win, 4, 4, rc == 0)), win


# ---- 6: timings -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_decode_timed_names_the_launch_resize(ctx, filt):
    import pjd_amd
    sc = [_scanned(golden_bytes(n), f) for n, f in (("big_640x480_420_q85", 16), ("ilsvrc_val_00000001", 0), ("gray_61x45", pjd_amd.F_FORCE_SEQUENTIAL))]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        _set(b, [(224, 224)] * 3, [W(10, 20, 250, 200, flip=True), W(vw=256, vh=256, ox=16, oy=16), None], filt == "antialias")
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize", per
        assert total >= per["resize"]


# ---- 7: the torch side, in a child process (tests/resize_window_torch_cases.py imports torch first) --------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "resize_window_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_decode_resized_batch_tensor_with_crops_and_flips():
    """32 synthetic ragged pictures, seeded crops and flips -> uint8[32, 3, 64, 64] equal to the model (prescale=False), and with
    prescale=True equal to the model over the box picture and window_at_scale."""
    _torch_case("crops_and_flips")


def test_decode_normalized_batch_tensor_resize_short_channels_last():
    _torch_case("resize_short_normalized")
