"""The antialiased resize on decode (pjd_batch_set_resize_filter, PJD_RESIZE_ANTIALIAS) on the GPU (run with -m gpu on an MI355X).
Every expectation is tests/resize_aa_model.py -- the numpy model of the arithmetic include/pjd.h specifies -- over the box filter of
the oracle's picture, transposed for planar, and every comparison is byte (bit, for floats) equality; never something this library
resized.  Only the progressive frame, which has no oracle, takes this library's own full-size decode as the source."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_corpus as G
import normalize_model as nm
import resize_aa_model as aa
import resize_model
from conftest import golden_bytes, ROOT
from test_gpu_resize import HUFF_ERR, MANIFEST, SCALES, VALID, _scanned
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}


def expected(rgb, s, tw, th, planar):
    """The model over the box filter of a full-size H x W x 3 picture; (3, th, tw) for planar."""
    out = aa.resize(box(rgb, s), tw, th)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if planar else out


def target_of(k, sw, sh):
    """The targets the fixtures cycle through, (tw, th) for a decode size of sw x sh: 1 x 1 where the 16x limit allows it (else the
    smallest target it allows), 7 x 5 clamped to the limit, the identity, one axis up with the other down."""
    lw, lh = -(-sw // 16), -(-sh // 16)
    return [(lw, lh), (max(7, lw), max(5, lh)), (sw, sh), (2 * sw + 3, sh // 2 + 1)][k % 4]


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


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
def oracle(port):
    out = {}
    for n in VALID:
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    return out


@pytest.fixture(scope="module")
def fixture_cases(oracle):
    """The cases of the all-fixtures batch, with the interleaved expectation of each computed once:
    [(fixture, scale flags, (th, tw), status, th x tw x 3 picture)]."""
    out = []
    for k, n in enumerate(VALID):
        flags, s = SCALES[k % 4]
        sw, sh = -(-MANIFEST[n]["dims"][0] // s), -(-MANIFEST[n]["dims"][1] // s)
        tw, th = target_of(k // 4 + k % 4, sw, sh)
        out.append((n, flags, (th, tw), oracle[n][0], expected(oracle[n][1], s, tw, th, False)))
    assert {(k // 4 + k % 4) % 4 for k in range(len(VALID)) if k % 4 == 0} == {0, 1, 2, 3}, "every pre-scale meets every target"
    assert any((th, tw) == (1, 1) for _, _, (th, tw), _, _ in out) and any(k % 4 == 0 and min(t) > 1 for k, (_, _, t, _, _) in enumerate(out)), \
        "1 x 1 is met, and so is a picture too large for it"
    return out


# ---- 1: every fixture in one batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_fixture_antialiased_in_one_batch(ctx, fixture_cases, mode, fmt):
    """All decodable fixtures (every sampling mode, grey, odd sizes, wrap_*, restart intervals, entropy errors), pre-scales 1, 1/2,
    1/4, 1/8 round-robin, the targets of target_of: byte equality with the model, the oracle's statuses, the sizes of set_resize."""
    import pjd_amd
    planar = fmt == "planar"
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    scanned = [_scanned(golden_bytes(n), flags | extra) for n, flags, _, _, _ in fixture_cases]
    sizes = [t for _, _, t, _, _ in fixture_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize(sizes)
        before = b.info()["device_bytes"]
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
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
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
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
        scanned.append(sc); sizes.append((th, tw)); want.append((n, oracle[n][0], expected(oracle[n][1], s, tw, th, False)))
    with ctx.batch([x.desc for x in scanned], pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload(); b.decode()
        outs, st = b.download()
    for (n, status, pic), o, got_st in zip(want, outs, st):
        assert got_st == status != 0, n
        assert np.array_equal(o, pic), n


# ---- 3: geometry the tiling can get wrong ---------------------------------------------------------------------------------------------
# (w, h, seed) of a synthetic picture -> (tw, th)
GEOMETRY = [((600, 40, 71), (259, 5)),                     # crosses a 256-column tile, a ragged last lane group (259 = 256 + 3)
            ((40, 600, 72), (5, 259)),                     # 33 row tiles, every one with taps beyond its own rows
            ((64, 64, 73), (4, 4)),                        # exactly 16x: 32 taps on both axes
            ((300, 20, 74), (257, 9)),                     # barely shrinking along x: a second tile of one column and one row
            ((31, 23, 75), (300, 41))]                     # growing: two taps, many target rows per source row


@pytest.fixture(scope="module")
def geometry_cases(port):
    synth = _synth()
    out = []
    for (w, h, seed), (tw, th) in GEOMETRY:
        data = synth.make(w, h, seed, 90, synth.SUB_444)
        out.append((data, (th, tw), aa.resize(port.decode(data)["rgb"], tw, th)))
    return out


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_tile_edges_and_the_tap_limit(ctx, geometry_cases, fmt):
    import pjd_amd
    planar = fmt == "planar"
    scanned = [_scanned(data, 0) for data, _, _ in geometry_cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, t, _ in geometry_cases])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0] * len(geometry_cases)
    for (_, (th, tw), want), o in zip(geometry_cases, outs):
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
        bad = np.argwhere(o != want)
        assert o.shape == want.shape and bad.size == 0, (tw, th, "first differing sample", bad[0].tolist(), "differing", len(bad))


def test_a_picture_past_16x_is_refused_and_named(ctx):
    """65 x 64 -> 4 x 4 is past the limit along x (64 x 65 along y); the batch is left as it was: bilinear."""
    import pjd_amd
    synth = _synth()
    L = pjd_amd.dev_lib()
    ok = _scanned(synth.make(64, 64, 73, 90, synth.SUB_444), 0)
    for w, h in ((65, 64), (64, 65)):
        bad = _scanned(synth.make(w, h, 76, 90, synth.SUB_444), 0)
        with ctx.batch([ok.desc, bad.desc, ok.desc], pjd_amd.OUT_RGB8) as b:
            b.set_resize([(4, 4)] * 3)
            assert L.pjd_batch_set_resize_filter(b._h, pjd_amd.RESIZE_ANTIALIAS) == E_ARG
            assert b"picture 1" in L.pjd_last_error(ctx._h) and b"16x" in L.pjd_last_error(ctx._h)
            with ctx.batch([ok.desc, bad.desc, ok.desc], pjd_amd.OUT_RGB8) as plain:
                plain.set_resize([(4, 4)] * 3)
                plain.upload(); plain.decode()
                want, _ = plain.download()
            b.upload(); b.decode()
            outs, st = b.download()
            assert st == [0, 0, 0] and all(np.array_equal(o, p) for o, p in zip(outs, want))
    # behind the 1/2 pre-scale the same picture is inside the limit
    half = _scanned(synth.make(65, 64, 76, 90, synth.SUB_444), pjd_amd.F_SCALE_1_2)
    with ctx.batch([half.desc], pjd_amd.OUT_RGB8) as b:
        b.set_resize([(4, 4)])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)


LIMITS = [("w65535x8_444", (40000, 1)), ("h8x65535_444_ri1", (1, 40000))]


@pytest.fixture(scope="module")
def limit_cases(port):
    out = []
    for name, (tw, th) in LIMITS:
        rgb = port.decode(G.oracle_bytes(name))["rgb"]
        out.append((name, (th, tw), aa.resize(rgb, tw, th)))
    return out


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_the_dimension_limits(ctx, limit_cases, fmt):
    """65535 samples along x and along y to 40000: (2i + 1) * sn passes 2^32, 157 column tiles, 5000 row tiles."""
    import pjd_amd
    planar = fmt == "planar"
    scanned = []
    for name, _, _ in limit_cases:
        s = pjd_amd.Scanned(G.jpeg(name), name + ".jpg")
        assert s.valid
        s.desc.flags = int(s.desc.flags) | G.flags(name)
        scanned.append(s)
    with ctx.batch([s.desc for s in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, t, _ in limit_cases])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0, 0]
    for (name, (th, tw), want), o in zip(limit_cases, outs):
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
        bad = np.argwhere(o != want)
        assert o.shape == want.shape and bad.size == 0, (name, "first differing sample", bad[0].tolist(), "differing", len(bad))


# ---- 4: bound, unaligned output on a captured graph; normalised output ------------------------------------------------------------------
BOUND = [("wrap_420_q65535", (9, 257)), ("env_61x45_444_q85_opt", (45, 61)), ("wrap_gray_q65535", (4, 259)), ("noise_80x96_422_q50_opt", (17, 7)),
         ("big_640x480_420_q85", (224, 224))]


@pytest.fixture(scope="module")
def bound_cases(oracle):
    return [(n, t, oracle[n][0], aa.resize(oracle[n][1], t[1], t[0])) for n, t in BOUND]


@pytest.mark.parametrize("dtype", [0] + DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_unaligned_output_on_a_captured_graph(ctx, bound_cases, fmt, dtype):
    """Pictures bound into device memory that holds a known pattern (a donor batch's decoded picture), uint8 pictures 1, 2 and 3
    bytes off a dword, float pictures an odd number of elements off: element-aligned and no more.  The decode is captured and
    replayed three times; then every picture is the model's (normalised by tests/normalize_model.py, bit for bit) and every
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
        assert mem % 256 == 0
        sc = [_scanned(golden_bytes(n), 0) for n, _, _, _ in bound_cases]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize([t for _, t, _, _ in bound_cases])
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
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
        want = nm.normalize(u8, dtype, scale, bias) if dtype else u8
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
        assert got_st == status and size == want.nbytes, n
        assert o.shape == want.shape and o.tobytes() == want.tobytes(), (n, fmt, DT_NAME[dtype])
        assert after[off:off + size].tobytes() == want.tobytes(), n
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_normalized_output_is_the_normalize_model_over_the_antialias_model(ctx, fixture_cases, fmt, dtype):
    """Every fourth fixture case (all four targets, the pre-scales, an entropy error among them) in the library's own buffer: aligned
    vector stores, where the bound test has element stores."""
    import pjd_amd
    from pjd_amd import tensors
    planar = fmt == "planar"
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    cases = fixture_cases[::5]
    assert {(k // 4 + k % 4) % 4 for k in range(0, len(fixture_cases), 5)} == {0, 1, 2, 3} and len({f for _, f, _, _, _ in cases}) == 4
    scanned = [_scanned(golden_bytes(n), flags) for n, flags, _, _, _ in cases]
    with ctx.batch([x.desc for x in scanned], _fmt(planar)) as b:
        b.set_resize([t for _, _, t, _, _ in cases])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.set_normalize(dtype, scale, bias)
        b.upload(); b.decode()
        outs, st = b.download()
    for (n, flags, (th, tw), status, u8), o, got_st in zip(cases, outs, st):
        want = nm.normalize(u8, dtype, scale, bias)
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
        assert got_st == status, n
        assert o.shape == want.shape and o.dtype == want.dtype and np.array_equal(nm.bits(o), nm.bits(want)), (n, flags, tw, th)


# ---- 5: call order ------------------------------------------------------------------------------------------------------------------------
def test_set_resize_filter_state_and_argument_errors(ctx):
    import pjd_amd
    L = pjd_amd.dev_lib()
    AA, BL = pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BILINEAR
    sc = [_scanned(golden_bytes(n), 0) for n in ("env_61x45_420_q100_opt", "gray_33x70")]
    descs = [x.desc for x in sc]
    sizes = [(20, 30), (31, 17)]
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.pjd_batch_set_resize_filter(None, AA) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # before set_resize
        assert L.pjd_batch_set_resize_filter(b._h, BL) == E_STATE
        b.set_resize(sizes)
        for bad in (2, -1, 255):
            assert L.pjd_batch_set_resize_filter(b._h, bad) == E_ARG                  # an unknown filter
            assert b"unknown filter" in L.pjd_last_error(ctx._h)
        assert L.pjd_batch_set_resize_filter(b._h, AA) == 0
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # twice
        assert L.pjd_batch_set_resize_filter(b._h, BL) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_resize_filter(b._h, BL) == 0
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # twice, the first one bilinear
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F16, one, one) == 0
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # after set_normalize
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, pjd_amd.DT_F32, one, one) == 0         # which sets the identity resize itself
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize(sizes)
        b.upload()
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # after upload
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize(sizes)
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                 # after bind_output
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        w, h = (C.c_uint32 * 2)(30, 17), (C.c_uint32 * 2)(20, 31)
        assert L.pjd_batch_set_resize(b._h, w, h) == E_ARG                            # a BMP batch is never resized ...
        assert L.pjd_batch_set_resize_filter(b._h, AA) == E_STATE                     # ... so it has no filter to choose
    with pytest.raises(pjd_amd.PjdError):
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.set_resize_filter(AA)


# ---- 6: the bilinear paths are what they were ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_bilinear_set_explicitly_equals_no_call(ctx, oracle, fmt):
    import pjd_amd
    planar = fmt == "planar"
    names = ["big_640x480_420_q85", "env_61x45_444_q85_opt", "gray_33x70", "wrap_420_q65535"]
    sizes = [(224, 224), (9, 257), (70, 33), (5, 7)]
    res = []
    for explicit in (False, True):
        sc = [_scanned(golden_bytes(n), 0) for n in names]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize(sizes)
            if explicit:
                b.set_resize_filter(pjd_amd.RESIZE_BILINEAR)
            b.upload(); b.decode()
            res.append(b.download() + (b.info()["device_bytes"],))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    for n, (th, tw), a, c in zip(names, sizes, res[0][0], res[1][0]):
        want = resize_model.resize(oracle[n][1], tw, th)
        want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
        assert np.array_equal(a, c) and np.array_equal(a, want), n


# ---- 7: timings, the fallback re-run -------------------------------------------------------------------------------------------------
def test_decode_timed_names_the_launch_resize(ctx):
    import pjd_amd
    sc = [_scanned(golden_bytes(n), f) for n, f in (("big_640x480_420_q85", 16), ("ilsvrc_val_00000001", 0), ("gray_61x45", pjd_amd.F_FORCE_SEQUENTIAL))]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize([(224, 224)] * 3)
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize", per
        assert total >= per["resize"]


# ---- 8: a progressive frame -------------------------------------------------------------------------------------------------------------
def test_progressive_frame_antialiased_is_the_model_over_its_full_picture(ctx):
    import io
    PIL = pytest.importorskip("PIL.Image")
    import pjd_amd
    rng = np.random.default_rng(5)
    w, h = 101, 77
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(xx / 9.0), 127 + 90 * np.cos(yy / 17.0), (xx + yy) * 255 / (w + h)], -1) + rng.normal(0, 12, (h, w, 3))
    bio = io.BytesIO()
    PIL.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(bio, "JPEG", quality=85, subsampling=2, progressive=True)
    full_sc = _scanned(bio.getvalue(), 0, options=pjd_amd.SCAN_PROGRESSIVE)
    assert int(full_sc.desc.n_scans) >= 2
    full, st = ctx.decode([full_sc.desc], pjd_amd.OUT_RGB8)
    assert st == [0]
    for planar in (False, True):
        sc = [_scanned(bio.getvalue(), f, options=pjd_amd.SCAN_PROGRESSIVE) for f in (0, pjd_amd.F_SCALE_1_2)]
        sizes = [(20, 31), (30, 41)]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize(sizes)
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
            b.upload(); b.capture(); b.decode()
            outs, st = b.download()
        assert st == [0, 0]
        for o, s, (th, tw) in zip(outs, (1, 2), sizes):
            assert np.array_equal(o, expected(full[0], s, tw, th, planar)), (s, planar)


# ---- 9: the torch side, in a child process (tests/resize_aa_torch_cases.py imports torch first) ---------------------------------------
def _torch_case(case, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "resize_aa_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_decode_resized_batch_tensor_antialiased():
    """64 synthetic pictures of different sizes -> ONE uint8[64, 3, 224, 224] torch tensor equal to the model, with the pre-scale and
    without it."""
    _torch_case("resized_batch_tensor")


def test_decode_normalized_batch_tensor_antialiased_channels_last():
    _torch_case("normalized_channels_last")
