"""Resize on decode (pjd_batch_set_resize) on the GPU (run with -m gpu on an MI355X): every back end (lane streams, picture groups,
exact kernel, progressive frames), both output formats, every pre-scale, bound and unbound, captured graphs, the torch side
(pjd_amd.tensors.decode_resized_batch_tensor).  The expected picture is always tests/resize_model.py -- the numpy model of the
arithmetic include/pjd.h specifies -- over the box filter of the oracle's picture, transposed for planar; never something this
library resized.  Where no oracle exists (progressive frames) and for the 1024-picture batch the source is this library's own
full-size PJD_OUT_RGB8 decode, which the other GPU suites pin to the oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_model
from conftest import golden_bytes, ROOT
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
HUFF_ERR = sorted(k for k in VALID if MANIFEST[k]["huff_ok"] == 0)
SCALES = [(0, 1), (16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)
E_ARG, E_STATE = -3, -5


def expected(rgb, s, tw, th, planar):
    """resize_model over the box filter of a full-size H x W x 3 picture; (3, th, tw) for planar."""
    out = resize_model.resize(box(rgb, s), tw, th)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if planar else out


def target_of(k, sw, sh):
    """The targets the fixtures cycle through: (tw, th) for the k-th picture, whose decode size is sw x sh."""
    return [(1, 1), (7, 5), (224, 224), (sw, sh), (2 * sw + 3, sh // 2 + 1)][k % 5]


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


def _scanned(data, flags, options=0):
    import pjd_amd
    s = pjd_amd.Scanned(data, options=options)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


# ---- 1: every fixture in one batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_every_fixture_resized_in_one_batch(ctx, oracle, mode, fmt):
    """All decodable fixtures (every sampling mode, grey, odd sizes, wrap_*, restart intervals, div_rst_*, entropy errors), pre-scales
    1, 1/2, 1/4, 1/8 round-robin, targets cycling through 1x1, 7x5, 224x224, the identity and (2*sw+3) x (sh//2+1): byte equality
    with the model over the box of the oracle's picture, the oracle's statuses, sizes and shapes as include/pjd.h states them."""
    import pjd_amd
    planar = fmt == "planar"
    out_fmt = pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    scanned, scale, sizes = [], [], []
    for k, n in enumerate(VALID):
        flags, s = SCALES[k % 4]
        scanned.append(_scanned(golden_bytes(n), flags | extra))
        scale.append(s)
        sw, sh = -(-MANIFEST[n]["dims"][0] // s), -(-MANIFEST[n]["dims"][1] // s)
        assert (sw, sh) == pjd_amd.scaled_dims(scanned[-1].desc.width, scanned[-1].desc.height, flags)
        tw, th = target_of(k // 4 + k % 4, sw, sh)
        sizes.append((th, tw))
    assert {target_of(k // 4 + k % 4, 2, 2) for k in range(len(VALID)) if k % 4 == 0} == {target_of(j, 2, 2) for j in range(5)}, "every pre-scale meets every target"
    with ctx.batch([x.desc for x in scanned], out_fmt) as b:
        b.set_resize(sizes)
        for i, (th, tw) in enumerate(sizes):
            assert b.output_size(i) == 3 * tw * th
            assert b.output_shape(i) == ((3, th, tw) if planar else (th, tw, 3))
            assert b.output_offset(i) % 256 == 0
        assert b.packed_size() >= b.output_offset(b.n - 1) + b.output_size(b.n - 1)
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    if mode == "exact":
        assert info["n_sequential"] == len(scanned)
    assert info["out_bytes"] == sum(3 * tw * th for th, tw in sizes)
    assert info["pixels"] == sum(int(x.desc.width) * int(x.desc.height) for x in scanned)
    for n, s, (th, tw), o, status in zip(VALID, scale, sizes, outs, st):
        want = expected(oracle[n][1], s, tw, th, planar)
        assert status == oracle[n][0], (n, s)
        assert o.shape == want.shape and np.array_equal(o, want), (n, s, tw, th, int(np.abs(o.astype(int) - want).max()))


# ---- 2: entropy-coding errors -----------------------------------------------------------------------------------------------------
def test_entropy_error_fixtures_keep_status_and_resize_the_partial_picture(ctx, oracle):
    import pjd_amd
    assert HUFF_ERR
    for k, n in enumerate(HUFF_ERR):
        for flags, s in SCALES:
            sc = _scanned(golden_bytes(n), flags)
            sw, sh = pjd_amd.scaled_dims(sc.desc.width, sc.desc.height, flags)
            tw, th = target_of(k + s, sw, sh)
            for out_fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_RGB8_PLANAR):
                with ctx.batch([sc.desc], out_fmt) as b:
                    b.set_resize([(th, tw)])
                    b.upload(); b.decode()
                    outs, st = b.download()
                assert st[0] == oracle[n][0] != 0, (n, s)
                assert np.array_equal(outs[0], expected(oracle[n][1], s, tw, th, out_fmt == pjd_amd.OUT_RGB8_PLANAR)), (n, s, tw, th)


# ---- 3: the identity target -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_identity_target_equals_the_unresized_batch(ctx, fmt):
    import pjd_amd
    out_fmt = pjd_amd.OUT_RGB8_PLANAR if fmt == "planar" else pjd_amd.OUT_RGB8
    scanned = [_scanned(golden_bytes(n), SCALES[k % 4][0]) for k, n in enumerate(VALID)]
    descs = [x.desc for x in scanned]
    plain, st_plain = ctx.decode(descs, out_fmt)
    with ctx.batch(descs, out_fmt) as b:
        b.set_resize([tuple(reversed(pjd_amd.scaled_dims(d.width, d.height, d.flags))) for d in descs])
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == st_plain
    for n, o, p in zip(VALID, outs, plain):
        assert o.shape == p.shape and np.array_equal(o, p), n


# ---- 4: the benchmark's workload --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan_mode", [0, 1])
def test_cfg3_batch_resized_to_224(port, plan_mode):
    """1024 ImageNet-like pictures, each pre-scaled by pick_scale_flags and resized to 224 x 224: capture, decode, download, two more
    decodes, download, packed download -- all equal to the model over the box of this library's own full-size decode, six of
    them to the model over the oracle; as many fallbacks as the unresized batch."""
    import pjd_amd
    from pjd_amd import tensors
    synth = _synth()
    jpegs = synth.cfg3_imagenet_like(1024, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    c = pjd_amd.Context(0, plan_mode=plan_mode)
    try:
        full_sc = [_scanned(j, 0) for j in jpegs]
        with c.batch([x.desc for x in full_sc]) as b:
            b.upload(); b.decode()
            full, st_full = b.download()
            fb_full = b.info()["n_fallback"]
        flags = [tensors.pick_scale_flags(x.desc.width, x.desc.height, 224, 224) for x in full_sc]
        assert len(set(flags)) > 1
        sc = [_scanned(j, f) for j, f in zip(jpegs, flags)]
        with c.batch([x.desc for x in sc]) as b:
            b.set_resize([(224, 224)] * 1024)
            b.upload(); b.capture()
            b.decode()
            outs, st = b.download()
            info = b.info()
            b.decode(); b.decode()
            outs2, st2 = b.download()
            packed, st3 = b.download_packed()
        assert st == st_full and st2 == st and st3 == st
        assert info["n_fallback"] == fb_full and info["plan_mode"] == plan_mode
        assert info["out_bytes"] == 1024 * 3 * 224 * 224
        for i in range(1024):
            want = expected(full[i], 1 << (flags[i] >> 4), 224, 224, False)
            assert np.array_equal(outs[i], want), i
            assert np.array_equal(outs2[i], want), i
            assert np.array_equal(packed[i], want.reshape(-1)), i
        for i in (0, 1, 2, 3, 513, 1022):
            assert np.array_equal(outs[i], expected(port.decode(jpegs[i])["rgb"], 1 << (flags[i] >> 4), 224, 224, False)), i
    finally:
        c.close()


# ---- 5: error returns -------------------------------------------------------------------------------------------------------------
def _u32(v):
    return (C.c_uint32 * len(v))(*v)


def test_set_resize_error_returns(ctx, oracle):
    import pjd_amd
    from pjd_amd import parallel
    L = pjd_amd.dev_lib()
    names = ["env_61x45_420_q100_opt", "gray_33x70", "rst4_128x96_444"]
    sc = [_scanned(golden_bytes(n), 0) for n in names]
    descs = [x.desc for x in sc]
    ok_w, ok_h = _u32([10, 20, 30]), _u32([11, 21, 31])
    assert L.pjd_batch_set_resize(None, ok_w, ok_h) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_set_resize(b._h, ok_w, ok_h) == E_ARG                      # a BMP batch
        assert b"BMP" in L.pjd_last_error(ctx._h)
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize(b._h, None, ok_h) == E_ARG
        assert L.pjd_batch_set_resize(b._h, ok_w, None) == E_ARG
        for bad in (0, 65536):
            assert L.pjd_batch_set_resize(b._h, _u32([10, bad, 30]), ok_h) == E_ARG
            assert b"picture 1" in L.pjd_last_error(ctx._h)
            assert L.pjd_batch_set_resize(b._h, ok_w, _u32([11, 21, bad])) == E_ARG
            assert b"picture 2" in L.pjd_last_error(ctx._h)
        # every refusal left the batch as it was: it decodes at its own sizes
        assert [b.output_size(i) for i in range(3)] == [3 * 61 * 45, 3 * 33 * 70, 3 * 128 * 96]
        b.upload()
        assert L.pjd_batch_set_resize(b._h, ok_w, ok_h) == E_STATE                    # after upload
        b.decode()
        outs, st = b.download()
        for n, o, s in zip(names, outs, st):
            assert s == oracle[n][0] and np.array_equal(o, oracle[n][1]), n
    with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
        b.set_resize([(11, 10), (21, 20), (65535, 1)])                                # the largest dimension is accepted
        assert L.pjd_batch_set_resize(b._h, ok_w, ok_h) == E_STATE                    # a second call
        assert b.output_size(2) == 3 * 65535
    # a shard: its picture is only partly written
    whole = _scanned(golden_bytes("rst4_128x96_444"), 0)
    segs, ecs = whole.seg_offsets(), whole.ecs()
    f, c = parallel.segment_range(len(segs), 1, 2)
    lo = int(segs[f]); hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
    d, keep = parallel.shard_descriptor(whole.desc, segs, ecs[lo:hi], lo, 1, 2)
    assert int(d.shard_n_segs) != 0
    with ctx.batch([descs[0], d], pjd_amd.OUT_RGB8) as b:
        assert L.pjd_batch_set_resize(b._h, _u32([8, 8]), _u32([8, 8])) == E_ARG
        assert b"picture 1" in L.pjd_last_error(ctx._h) and b"shard" in L.pjd_last_error(ctx._h)
    # bind_output: its ranges are the resized pictures'.  Device memory without torch: the output buffer of a donor batch.
    donor_sc = _scanned(golden_bytes("big_640x480_420_q85"), 0)
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        mem, cap = donor.device_output(0), donor.output_size(0)
        with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
            sizes = [(50, 40), (9, 100), (64, 64)]
            b.set_resize(sizes)
            last_end = b.output_offset(2) + b.output_size(2)
            assert b.output_size(2) == 3 * 64 * 64 and last_end <= cap
            assert L.pjd_batch_bind_output(b._h, C.c_void_p(mem), last_end - 1, None) == E_ARG      # one byte short of the resized pictures
            own = b.info()["device_bytes"]
            b.bind_output(mem, last_end)
            assert b.info()["device_bytes"] == own - b.packed_size()                   # the result buffer went back, the intermediate stays
            assert b.device_output(1) == mem + b.output_offset(1)
            b.upload(); b.decode()
            outs, st = b.download()
            for n, (th, tw), o, s in zip(names, sizes, outs, st):
                assert s == oracle[n][0] and np.array_equal(o, expected(oracle[n][1], 1, tw, th, True)), n
        with ctx.batch(descs, pjd_amd.OUT_RGB8) as b:
            b.bind_output(mem, cap)
            assert L.pjd_batch_set_resize(b._h, ok_w, ok_h) == E_STATE                # after bind_output


# ---- 6: timings -------------------------------------------------------------------------------------------------------------------
def test_decode_timed_lists_the_resize_kernel(ctx):
    import pjd_amd
    sc = [_scanned(golden_bytes(n), f) for n, f in (("big_640x480_420_q85", 16), ("ilsvrc_val_00000001", 0), ("gray_61x45", pjd_amd.F_FORCE_SEQUENTIAL))]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_resize([(224, 224)] * 3)
        b.upload()
        per, total = b.decode_timed()
        assert "resize" in per and per["resize"] > 0 and list(per)[-1] == "resize", per
        assert total >= per["resize"]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.upload()
        per, _ = b.decode_timed()
        assert "resize" not in per


# ---- 7: progressive frames --------------------------------------------------------------------------------------------------------
def test_progressive_frame_resized_is_the_model_over_its_full_picture(ctx):
    import io
    PIL = pytest.importorskip("PIL.Image")
    import pjd_amd
    rng = np.random.default_rng(5)
    w, h, sub = 101, 77, 2
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(xx / 9.0), 127 + 90 * np.cos(yy / 17.0), (xx + yy) * 255 / (w + h)], -1) + rng.normal(0, 12, (h, w, 3))
    bio = io.BytesIO()
    PIL.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(bio, "JPEG", quality=85, subsampling=sub, progressive=True)
    full_sc = _scanned(bio.getvalue(), 0, options=pjd_amd.SCAN_PROGRESSIVE)
    assert int(full_sc.desc.n_scans) >= 2
    full, st = ctx.decode([full_sc.desc], pjd_amd.OUT_RGB8)
    assert st == [0]
    for out_fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_RGB8_PLANAR):
        sc = [_scanned(bio.getvalue(), f, options=pjd_amd.SCAN_PROGRESSIVE) for f in (0, pjd_amd.F_SCALE_1_2)]
        sizes = [(224, 224), (30, 41)]
        with ctx.batch([x.desc for x in sc], out_fmt) as b:
            b.set_resize(sizes)
            b.upload(); b.capture(); b.decode()
            outs, st = b.download()
        assert st == [0, 0]
        for o, s, (th, tw) in zip(outs, (1, 2), sizes):
            assert np.array_equal(o, expected(full[0], s, tw, th, out_fmt == pjd_amd.OUT_RGB8_PLANAR)), (s, out_fmt)


# ---- 8-9: the torch side, in child processes (tests/resize_torch_cases.py imports torch first) ----------------------------------------
def _torch_case(case, *args, timeout=1200):
    r = subprocess.run([sys.executable, os.path.join(HERE, "resize_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_decode_resized_batch_tensor_on_the_cfg3_batch():
    """1024 ImageNet-like pictures of different sizes -> ONE uint8[1024, 3, 224, 224] torch tensor equal to the model, a view of one
    buffer; with and without prescale; the caller's descriptors unchanged."""
    _torch_case("resized_batch_tensor")


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_unaligned_bound_output_and_guard_bytes(fmt, mode):
    """Resized pictures bound at base + 1 with odd gaps in a buffer filled with 0xA5: every picture is the model's, every other byte
    still 0xA5; after the whole buffer was overwritten and the captured graph replayed, every picture byte is rewritten."""
    _torch_case("guard_bytes", fmt, mode)
