"""Normalised float output (pjd_batch_set_normalize) on the GPU (run with -m gpu on an MI355X): the store paths of the three element
types in both layouts, with and without a resize, both back ends, bound output with guard bytes, subnormals / infinities / negative
values, the fused arithmetic, captured graphs, a ragged batch, the error returns, the torch side.  The expected bytes are always the
models over the oracle: the oracle's picture, the box pre-scale if flagged (test_gpu_scaled.box), tests/resize_model.py, then
tests/normalize_model.py -- never a uint8 picture this library made (case 10 apart, which says why)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import resize_model
from conftest import golden_bytes
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
# one fixture per sampling mode (4:4:4 at odd sizes, 4:2:2, 4:2:0, 4:4:0), one grey, one entropy-coding error (a partial picture with
# grey).  Chosen with the oracle so that their pictures hold (nearly) every level: test_level_coverage_of_the_store_path_cases.
FIXTURES = ["env_61x45_444_q85_opt", "noise_80x96_422_q50_opt", "wrap_420_q65535", "wrap_440_q65535", "wrap_gray_q65535", "err_truncated_eoi_420"]
# (th, tw): one pixel; a ragged lane; one tile exactly; one row and one column past a tile; ragged right edges of 1 and 3 pixels behind
# a full tile; an odd width (alternate planar rows off the vector alignment); None: the picture's own size
TARGETS = [(1, 1), (9, 5), (8, 256), (9, 257), (3, 259), (17, 7), None]
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(port):
    out = {}
    for n in FIXTURES:
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    assert out["err_truncated_eoi_420"][0] != 0
    return out


@pytest.fixture(scope="module")
def sets():
    from pjd_amd import tensors
    return nm.constant_sets(tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD))


@pytest.fixture(scope="module")
def store_cases(oracle):
    """The cases of test 1, computed once: [(fixture, (th, tw), expected uint8 picture th x tw x 3)]."""
    out = []
    for n in FIXTURES:
        rgb = oracle[n][1]
        for t in TARGETS:
            th, tw = t if t is not None else rgb.shape[:2]
            out.append((n, (th, tw), resize_model.resize(rgb, tw, th)))
    return out


def _scanned(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _fmt(planar):
    import pjd_amd
    return pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8


def _want(u8, dtype, scale, bias, planar):
    w = nm.normalize(u8, dtype, scale, bias)
    return np.ascontiguousarray(w.transpose(2, 0, 1)) if planar else w


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(nm.bits(got), nm.bits(want))


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ---- 1: the edges of the store paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_store_paths_at_tile_and_alignment_edges(ctx, oracle, sets, store_cases, fmt, dtype):
    planar = fmt == "planar"
    scale, bias = sets["imagenet"]
    es = nm.ESIZE[dtype]
    sc = [_scanned(golden_bytes(n)) for n, _, _ in store_cases]
    with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
        b.set_resize([t for _, t, _ in store_cases])
        b.set_normalize(dtype, scale, bias)
        for i, (_, (th, tw), _) in enumerate(store_cases):
            assert b.output_size(i) == 3 * tw * th * es
            assert b.output_shape(i) == ((3, th, tw) if planar else (th, tw, 3))
            assert b.output_offset(i) % 256 == 0
        assert b.packed_size() >= b.output_offset(b.n - 1) + b.output_size(b.n - 1)
        b.upload(); b.decode()
        outs, st = b.download()
        packed, st2 = b.download_packed()
        assert b.info()["out_bytes"] == sum(3 * tw * th * es for _, (th, tw), _ in store_cases)
    assert st == st2 == [oracle[n][0] for n, _, _ in store_cases]
    for (n, t, u8), o, p in zip(store_cases, outs, packed):
        want = _want(u8, dtype, scale, bias, planar)
        assert _same(o, want), (n, t, fmt, DT_NAME[dtype])
        assert p.tobytes() == want.tobytes(), (n, t)


# ---- 2: level coverage: a condition on the cases above ----------------------------------------------------------------------------
def test_level_coverage_of_the_store_path_cases(store_cases):
    seen = np.zeros((3, 256), bool)
    for _, _, u8 in store_cases:
        for c in range(3):
            seen[c][np.unique(u8[..., c])] = True
    counts = seen.sum(axis=1)
    print("levels met per channel:", counts.tolist())
    assert np.all(counts >= 200), counts


# ---- 3: no resize set -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt,dtype", [("planar", nm.DT_F16), ("rgb8", nm.DT_F32), ("rgb8", nm.DT_BF16)])
def test_normalize_without_a_resize_is_the_model_over_the_unresized_picture(ctx, oracle, sets, fmt, dtype, mode):
    import pjd_amd
    planar = fmt == "planar"
    scale, bias = sets["imagenet"]
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    flags = [(pjd_amd.F_SCALE_1_2, 2) if k % 2 else (0, 1) for k in range(2 * len(FIXTURES))]
    names = [FIXTURES[k // 2] for k in range(2 * len(FIXTURES))]
    sc = [_scanned(golden_bytes(n), f | extra) for n, (f, _) in zip(names, flags)]
    with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
        plain_sizes = [b.output_size(i) for i in range(b.n)]
        own = b.info()["device_bytes"]
        b.set_normalize(dtype, scale, bias)
        assert [b.output_size(i) for i in range(b.n)] == [s * nm.ESIZE[dtype] for s in plain_sizes]
        assert b.info()["device_bytes"] > own                                  # the intermediate stays, the result buffer is new
        ws, hs = (C.c_uint32 * b.n)(*([8] * b.n)), (C.c_uint32 * b.n)(*([8] * b.n))
        assert b.L.pjd_batch_set_resize(b._h, ws, hs) == E_STATE
        b.upload(); b.decode()
        outs, st = b.download()
        if mode == "exact":
            assert b.info()["n_sequential"] == b.n
    for n, (_, s), o, status in zip(names, flags, outs, st):
        assert status == oracle[n][0], n
        assert _same(o, _want(box(oracle[n][1], s), dtype, scale, bias, planar)), (n, s, fmt, DT_NAME[dtype], mode)


# ---- 4: bound output ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_bound_output_element_aligned_with_guard_bytes(ctx, oracle, sets, fmt, dtype):
    """Pictures bound into device memory that holds a known pattern (a donor batch's decoded picture: device memory without torch),
    the first at an offset of ONE element, the others an odd number of elements behind their predecessor: element-aligned, not
    vector-aligned.  After two decodes every picture is the model's and every byte outside the pictures still the donor's."""
    import pjd_amd
    planar = fmt == "planar"
    es = nm.ESIZE[dtype]
    scale, bias = sets["imagenet"]
    cases = [("wrap_420_q65535", (9, 257)), ("env_61x45_444_q85_opt", (45, 61)), ("wrap_gray_q65535", (3, 259)), ("noise_80x96_422_q50_opt", (17, 7))]
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        donor.upload(); donor.decode()
        (pattern,), _ = donor.download()
        pattern = pattern.reshape(-1).copy()
        mem, cap = donor.device_output(0), donor.output_size(0)
        assert mem % 256 == 0
        sc = [_scanned(golden_bytes(n)) for n, _ in cases]
        with ctx.batch([x.desc for x in sc], _fmt(planar)) as b:
            b.set_resize([t for _, t in cases])
            b.set_normalize(dtype, scale, bias)
            offs, pos = [], es
            for i in range(b.n):
                offs.append(pos)
                pos += b.output_size(i) + (2 * i + 1) * es
            assert pos <= cap and all(o % es == 0 for o in offs) and offs[0] % (4 * es) != 0
            # element alignment is required, and nothing beyond it
            for bad in ([1, 3] if es == 2 else [1, 2, 3, 6]):
                bad_offs = (C.c_uint64 * b.n)(*([offs[0] + bad] + offs[1:]))
                assert b.L.pjd_batch_bind_output(b._h, C.c_void_p(mem), cap, bad_offs) == E_ARG, bad
                assert b"element" in b.L.pjd_last_error(ctx._h) and b"picture 0" in b.L.pjd_last_error(ctx._h)
            assert b.L.pjd_batch_bind_output(b._h, C.c_void_p(mem + 1), cap - 1, None) == E_ARG          # the packed layout at an odd base
            own = b.info()["device_bytes"]
            b.bind_output(mem, cap, offs)
            assert b.info()["device_bytes"] == own - b.packed_size()
            assert [b.output_offset(i) for i in range(b.n)] == offs and b.device_output(1) == mem + offs[1]
            b.upload()
            for _ in range(2):
                b.decode(); b.sync()
            outs, st = b.download()
            sizes = [b.output_size(i) for i in range(b.n)]
        (after,), _ = donor.download()
        after = after.reshape(-1)
    covered = np.zeros(cap, bool)
    for (n, (th, tw)), o, off, size, status in zip(cases, outs, offs, sizes, st):
        want = _want(resize_model.resize(oracle[n][1], tw, th), dtype, scale, bias, planar)
        assert status == oracle[n][0]
        assert _same(o, want), (n, fmt, DT_NAME[dtype])
        assert after[off:off + size].tobytes() == want.tobytes(), n
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"


# ---- 5: special values on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["subnormal", "overflow", "negative"])
def test_subnormals_infinities_and_negative_values_on_the_device(ctx, oracle, sets, name):
    """A picture with every level; binary16 subnormals must come out as the model's (a flushed subnormal is a defect of the code)."""
    scale, bias = sets[name]
    rgb = oracle["wrap_420_q65535"][1]
    assert all(len(np.unique(rgb[..., c])) == 256 for c in range(3))
    sc = _scanned(golden_bytes("wrap_420_q65535"))
    for dtype in DTYPES:
        for planar in (True, False):
            with ctx.batch([sc.desc], _fmt(planar)) as b:
                b.set_normalize(dtype, scale, bias)
                b.upload(); b.decode()
                (o,), _ = b.download()
            want = _want(rgb, dtype, scale, bias, planar)
            if name == "subnormal" and dtype == nm.DT_F16:
                h = nm.bits(want)
                assert np.count_nonzero(((h & 0x7c00) == 0) & ((h & 0x3ff) != 0)) > 0
            assert _same(o, want), (name, DT_NAME[dtype], planar)


# ---- 6: the fused arithmetic on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_f32_with_the_imagenet_constants_is_the_fused_result(ctx, oracle, sets, fmt):
    """Byte-exact binary32 with the ImageNet constants: what a multiply followed by an add would not give (the unfused float32 picture
    differs from the model on a large share of the samples; tests/test_normalize_cpu.py counts the levels)."""
    planar = fmt == "planar"
    scale, bias = sets["imagenet"]
    rgb = oracle["wrap_420_q65535"][1]
    sc = _scanned(golden_bytes("wrap_420_q65535"))
    with ctx.batch([sc.desc], _fmt(planar)) as b:
        b.set_normalize(nm.DT_F32, scale, bias)
        b.upload(); b.decode()
        (o,), _ = b.download()
    want = _want(rgb, nm.DT_F32, scale, bias, planar)
    unfused = (rgb.astype(np.float32) * scale[None, None, :]).astype(np.float32) + bias[None, None, :]
    unfused = np.ascontiguousarray(unfused.transpose(2, 0, 1)) if planar else unfused
    assert np.count_nonzero(nm.bits(unfused) != nm.bits(want)) > want.size // 4
    assert _same(o, want)


# ---- 7: graph and timing -----------------------------------------------------------------------------------------------------------
def test_captured_graph_timings_and_out_bytes(ctx, oracle, sets):
    import pjd_amd
    scale, bias = sets["imagenet"]
    sizes = [(33, 47), (224, 224), (5, 300), (64, 64), (1, 1), (96, 64)]
    sc = [_scanned(golden_bytes(n), pjd_amd.F_SCALE_1_2 if k == 1 else 0) for k, n in enumerate(FIXTURES)]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize(sizes)
        b.set_normalize(nm.DT_BF16, scale, bias)
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize" and total >= per["resize"], per
        first, st = b.download()
        b.capture()
        for _ in range(3):
            b.decode()
            outs, st2 = b.download()
            assert st2 == st
            for o, f in zip(outs, first):
                assert o.tobytes() == f.tobytes()
        assert b.info()["out_bytes"] == sum(3 * tw * th * 2 for th, tw in sizes)
    for k, (n, (th, tw), o) in enumerate(zip(FIXTURES, sizes, first)):
        assert _same(o, _want(resize_model.resize(box(oracle[n][1], 2 if k == 1 else 1), tw, th), nm.DT_BF16, scale, bias, True)), n


# ---- 8: a ragged batch -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(oracle, sets):
    rng = np.random.default_rng(8)
    scale, bias = sets["imagenet"]
    names = [FIXTURES[k % len(FIXTURES)] for k in range(64)]
    sizes = [(int(rng.integers(1, 301)), int(rng.integers(1, 301))) for _ in range(64)]
    want = [_want(resize_model.resize(oracle[n][1], tw, th), nm.DT_F16, scale, bias, True) for n, (th, tw) in zip(names, sizes)]
    return names, sizes, want


@pytest.mark.parametrize("plan_mode", [0, 1])
def test_ragged_batch_of_64_pictures(oracle, sets, ragged, plan_mode):
    """64 pictures, each to a size of its own in 1..300: more pictures than a wave has lanes, tiles found by the prefix search."""
    import pjd_amd
    names, sizes, want = ragged
    scale, bias = sets["imagenet"]
    c = pjd_amd.Context(0, plan_mode=plan_mode)
    try:
        sc = [_scanned(golden_bytes(n)) for n in names]
        with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_resize(sizes)
            b.set_normalize(nm.DT_F16, scale, bias)
            b.upload(); b.decode()
            outs, st = b.download()
            assert b.info()["plan_mode"] == plan_mode
    finally:
        c.close()
    assert st == [oracle[n][0] for n in names]
    for i, (o, w) in enumerate(zip(outs, want)):
        assert _same(o, w), (i, names[i], sizes[i])


# ---- 9: error returns --------------------------------------------------------------------------------------------------------------
def test_set_normalize_error_returns(ctx, oracle, sets):
    import pjd_amd
    from pjd_amd import parallel
    L = pjd_amd.dev_lib()
    scale, bias = sets["imagenet"]
    ok_s, ok_b = _f3(scale), _f3(bias)
    err = lambda: L.pjd_last_error(ctx._h)
    names = ["env_61x45_444_q85_opt", "wrap_gray_q65535"]
    sc = [_scanned(golden_bytes(n)) for n in names]
    descs = [x.desc for x in sc]
    assert L.pjd_batch_set_normalize(None, nm.DT_F16, ok_s, ok_b) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, ok_s, ok_b) == E_ARG and b"BMP" in err()
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, None, ok_b) == E_ARG and b"null" in err()
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, ok_s, None) == E_ARG and b"null" in err()
        for bad_dt in (0, 4, -1):
            assert L.pjd_batch_set_normalize(b._h, bad_dt, ok_s, ok_b) == E_ARG and b"dtype" in err()
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert L.pjd_batch_set_normalize(b._h, nm.DT_F32, _f3([scale[0], bad, scale[2]]), ok_b) == E_ARG and b"finite" in err()
            assert L.pjd_batch_set_normalize(b._h, nm.DT_F32, ok_s, _f3([bias[0], bias[1], bad])) == E_ARG and b"finite" in err()
        # every refusal left the batch as it was
        assert [b.output_size(i) for i in range(2)] == [3 * 61 * 45, 3 * 88 * 56]
        b.set_normalize(nm.DT_F32, scale, bias)
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F32, ok_s, ok_b) == E_STATE and b"already" in err()        # the call twice
        assert [b.output_size(i) for i in range(2)] == [12 * 61 * 45, 12 * 88 * 56]
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.upload()
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, ok_s, ok_b) == E_STATE and b"upload" in err()           # after upload
        b.decode()
        outs, st = b.download()
        for n, o in zip(names, outs):
            assert np.array_equal(o, oracle[n][1]), n
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.bind_output(donor.device_output(0), donor.output_size(0))
            assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, ok_s, ok_b) == E_STATE and b"bind" in err()         # after bind
    # a shard: its picture is only partly written
    whole = _scanned(golden_bytes("rst4_128x96_444"))
    segs, ecs = whole.seg_offsets(), whole.ecs()
    f, c = parallel.segment_range(len(segs), 1, 2)
    lo = int(segs[f]); hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
    d, keep = parallel.shard_descriptor(whole.desc, segs, ecs[lo:hi], lo, 1, 2)
    assert int(d.shard_n_segs) != 0
    with ctx.batch([descs[0], d], pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_normalize(b._h, nm.DT_F16, ok_s, ok_b) == E_ARG
        assert b"picture 1" in err() and b"shard" in err()


# ---- 10: the torch side, in child processes (tests/normalize_torch_cases.py imports torch first) -------------------------------------
@pytest.mark.parametrize("channels_last", [0, 1])
def test_decode_normalized_batch_tensor(channels_last):
    """Shape, dtype and memory format for each dtype; bit for bit the model over decode_resized_batch_tensor's uint8 tensor -- the
    same P' by definition, which tests/test_gpu_resize.py pins to the oracle separately; equal statuses."""
    case = "normalized_batch_tensor"
    r = subprocess.run([sys.executable, os.path.join(HERE, "normalize_torch_cases.py"), case, str(channels_last)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])
