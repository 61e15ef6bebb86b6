"""Planar output (PJD_OUT_RGB8_PLANAR) and caller-owned output memory (pjd_batch_bind_output) on the GPU (run with -m gpu on an
MI355X): every back end (lane streams, picture groups, exact kernel, progressive frames), every scale, shards, split decode, the
pipelined batcher and the torch side (pjd_amd.tensors).  The expected picture is always the oracle's RGB picture -- through the box
filter of include/pjd.h for a scaled one -- transposed to (3, H, W); never something this library's own planar path produced.  Where
no oracle exists (progressive frames) and for the 1024-picture batch it is this library's PJD_OUT_RGB8 full-size decode, which the
other GPU suites pin to the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_bytes, ROOT
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
HUFF_ERR = sorted(k for k in VALID if MANIFEST[k]["huff_ok"] == 0)
SCALES = [(0, 1), (16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)
GUARD = ["env_1x1_444_q85", "env_1x1_420_q100", "env_17x9_420_q100", "env_17x9_422_q30_opt", "env_61x45_444_q85_opt",
         "env_61x45_420_q100_opt", "h1v2_45x61", "gray_61x45", "gray_33x70", "sym_frame_420_300x1_ri0", "sym_frame_444_1x300_ri1",
         "rstrow_200x150_444_opt", "err_truncated_eoi_420"]
E_ARG, E_STATE = -3, -5


def chw(rgb, s=1):
    """The expected planar picture: the box filter of an H x W x 3 picture, channels first."""
    return np.ascontiguousarray(box(rgb, s).transpose(2, 0, 1))


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(port):
    """name -> (status, full-size RGB) of the oracle for every decodable fixture"""
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


# ---- 1: every fixture at every scale in one planar batch, both back ends ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_fixtures_mixed_scale_planar_batch_match_transposed_oracle(ctx, oracle, mode):
    import pjd_amd
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    names, scanned = [], []
    for n in VALID:
        for flags, s in SCALES:
            names.append((n, s))
            scanned.append(_scanned(golden_bytes(n), flags | extra))
    with ctx.batch([x.desc for x in scanned], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    if mode == "exact":
        assert info["n_sequential"] == len(scanned)
    for (n, s), o, status in zip(names, outs, st):
        want = chw(oracle[n][1], s)
        assert status == oracle[n][0], (n, s)
        assert o.shape == want.shape and np.array_equal(o, want), (n, s, o.shape, want.shape)
    assert info["out_bytes"] == sum(3 * -(-int(x.desc.width) // s) * -(-int(x.desc.height) // s) for x, (_, s) in zip(scanned, names))
    assert info["pixels"] == sum(int(x.desc.width) * int(x.desc.height) for x in scanned)


# ---- 2: entropy-coding errors ----------------------------------------------------------------------------------------------------
def test_entropy_error_fixtures_keep_status_and_partial_picture(ctx, oracle):
    import pjd_amd
    assert HUFF_ERR
    for n in HUFF_ERR:
        for flags, s in SCALES:
            sc = _scanned(golden_bytes(n), flags)
            outs, st = ctx.decode([sc.desc], pjd_amd.OUT_RGB8_PLANAR)
            assert st[0] == oracle[n][0] != 0, (n, s)
            assert np.array_equal(outs[0], chw(oracle[n][1], s)), (n, s)


# ---- 3-7: everything that needs torch, in child processes ------------------------------------------------------------------------
# torch ships its own HIP runtime; torch and libpjd.so share ONE runtime -- and with it device pointers -- only when torch is loaded
# first ("Pictures as tensors").  By the time this file runs, earlier tests have loaded libpjd.so into the pytest
# process, so these cases run in a fresh process each: tests/planar_torch_cases.py imports torch before anything else.
def _torch_case(case, *args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(HERE, "planar_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("plan_mode", [0, 1])
def test_cfg3_batch_bound_to_a_torch_buffer(plan_mode):
    """1024 ImageNet-like pictures, scales round-robin, planar, written into a torch.uint8 buffer of the test's: equal to the
    transposed box of the same library's RGB8 full-size decode (six of them: of the oracle's), and again after the whole buffer
    was overwritten and the captured graph replayed -- every decode writes every byte; decode_to_tensors on the first 64."""
    _torch_case("cfg3_bound", plan_mode)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["planar", "rgb8"])
def test_no_byte_outside_the_picture_ranges_is_written(fmt, mode):
    """Pictures with awkward edges at every scale, bound with a 37-byte gap before the first and odd gaps (1, 3, 5, ...) between
    them, in a buffer pre-filled with 0xA5: every picture is the oracle's, every other byte is still 0xA5."""
    _torch_case("guard_bytes", fmt, mode)


def test_decode_to_batch_tensor():
    """64 synthetic pictures of one size (4:2:0, width not a multiple of 16) as ONE contiguous uint8[64,3,H,W] torch tensor."""
    _torch_case("batch_tensor")


def test_tensors_order_the_torch_stream_before_the_decode():
    """A buffer recycled by torch's caching allocator while kernels queued on torch's stream still read it is not overwritten
    early: pjd_amd.tensors drains torch's current stream before the library (on its own, non-blocking stream) writes."""
    _torch_case("stream_order")


def test_bind_output_error_returns():
    """BMP batch, after upload, short capacity, ranges beyond the capacity, overlapping offsets, host pointers: each with its code,
    and the batch still decodes into its own buffer."""
    _torch_case("bind_errors")


def test_device_bytes_of_a_bound_batch():
    _torch_case("device_bytes")


# ---- 8: shards and split decode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", [("rstrow_200x150_444_opt", 2), ("rst4_128x96_444", 4), ("rstrow_gray_100x60", 3)])
def test_shard_unions_planar(ctx, oracle, name, world):
    import pjd_amd
    from pjd_amd import parallel
    for flags, s in [(0, 1), (32, 4)]:
        sc = _scanned(golden_bytes(name), flags)
        segs, ecs = sc.seg_offsets(), sc.ecs()
        d0 = sc.desc
        want = chw(oracle[name][1], s)
        got = np.zeros_like(want)
        mcux = (d0.width + 7) // 8
        m = 8 // s                                                    # 1x1 luma: an MCU is 8 x 8 source pixels
        for r in range(world):
            f, c = parallel.segment_range(len(segs), r, world)
            lo = int(segs[f])
            hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
            d, keep = parallel.shard_descriptor(d0, segs, ecs[lo:hi], lo, r, world)
            outs, st = ctx.decode([d], pjd_amd.OUT_RGB8_PLANAR)
            assert st == [0] and outs[0].shape == want.shape
            m0, m1 = f * d0.restart_interval, min((f + c) * d0.restart_interval, mcux * ((d0.height + 7) // 8))
            for k in range(m0, m1):
                y0, x0 = (k // mcux) * m, (k % mcux) * m
                got[:, y0:y0 + m, x0:x0 + m] = outs[0][:, y0:y0 + m, x0:x0 + m]
        assert np.array_equal(got, want), (name, s)


def test_split_decode_planar_equals_one_device_and_oracle(ctx, oracle, monkeypatch):
    import pjd_amd
    monkeypatch.setenv("PJD_PIPE_ALLOW_DUP_DEVICES", "1")
    for name in ("rstrow_200x150_444_opt", "rst4_128x96_444", "rstrow_gray_100x60"):
        for flags, s in [(0, 1), (32, 4)]:
            sc = _scanned(golden_bytes(name), flags)
            whole, st = ctx.decode([sc.desc], pjd_amd.OUT_RGB8_PLANAR)
            want = chw(oracle[name][1], s)
            assert st == [0] and np.array_equal(whole[0], want), (name, s)
            for world in (1, 2, 3, 5):
                got, status, stats = pjd_amd.split_decode(sc.desc, [0] * world, pjd_amd.OUT_RGB8_PLANAR)
                assert status == 0 and stats["redone_whole"] == 0, (name, s, world)
                assert stats["n_ranks"] == min(world, int(sc.desc.n_segments)), (name, s, world, stats)
                assert got.shape == want.shape and np.array_equal(got, want), (name, s, world)
    pjd_amd.dev_lib().pjd_split_release()


# ---- 9: progressive frames ---------------------------------------------------------------------------------------------------------
def test_progressive_planar_is_the_transpose_of_rgb8(ctx):
    import io
    PIL = pytest.importorskip("PIL.Image")
    import pjd_amd
    rng = np.random.default_rng(5)
    for (w, h, sub) in [(101, 77, 2), (64, 48, 0), (33, 70, 1)]:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([127 + 100 * np.sin(xx / 9.0), 127 + 90 * np.cos(yy / 17.0), (xx + yy) * 255 / (w + h)], -1) + rng.normal(0, 12, (h, w, 3))
        bio = io.BytesIO()
        PIL.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(bio, "JPEG", quality=85, subsampling=sub, progressive=True)
        got = {}
        for fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_RGB8_PLANAR):
            descs = [_scanned(bio.getvalue(), flags, options=pjd_amd.SCAN_PROGRESSIVE) for flags in (0, pjd_amd.F_SCALE_1_4)]
            assert all(int(x.desc.n_scans) >= 2 for x in descs)
            outs, st = ctx.decode([x.desc for x in descs], fmt)
            assert st == [0, 0]
            got[fmt] = outs
        for k in range(2):
            assert np.array_equal(got[pjd_amd.OUT_RGB8_PLANAR][k], got[pjd_amd.OUT_RGB8][k].transpose(2, 0, 1)), (w, h, sub, k)


# ---- 10: pipelined batcher -----------------------------------------------------------------------------------------------------------
def test_pipeline_planar_sink_payloads(ctx, oracle):
    import threading
    import pjd_amd
    names = sorted(MANIFEST)
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            got[index] = (status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=[golden_bytes(n) for n in names], names=[n + ".jpg" for n in names], out_format=pjd_amd.OUT_RGB8_PLANAR,
                          batch_images=7, slots=2, sink=sink)
    assert st["n_decoded"] == len(VALID) and st["n_batch_failures"] == 0
    for i, n in enumerate(names):
        status, data = got[i]
        if MANIFEST[n]["rc"] != 0:
            assert status == -1 and data is None, n
            continue
        assert status == oracle[n][0], n
        assert np.array_equal(data, chw(oracle[n][1]).reshape(-1)), n


# ---- 11: a batch alone on an idle device -------------------------------------------------------------------------------------------
def test_planar_batch_of_80_replayed_on_an_idle_device():
    """A planar batch of 80 pictures, captured and replayed on an idle device (a child process of its own: nothing else of this suite
    is on the device): it takes the picture groups and comes out right."""
    code = f"""
import os, sys
sys.path.insert(0, {os.path.join(ROOT, "pim-jpeg-decoder_amd", "python")!r}); sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(ROOT, "tools")!r})
import numpy as np, pjd_amd, oracle_lib, synth
port = oracle_lib.Port()
jpegs = synth.cfg3_imagenet_like(80, seed=31, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
sc = [pjd_amd.Scanned(j) for j in jpegs]
ctx = pjd_amd.Context(0)
b = ctx.batch([s.desc for s in sc], pjd_amd.OUT_RGB8_PLANAR)
b.upload(); b.capture()
for rep in range(2):
    b.decode(); b.sync()
    assert b.decode_chains() == 3, (rep, b.decode_chains())
outs, st = b.download()
bad = [k for k in range(len(jpegs)) if st[k] != 0 or not np.array_equal(outs[k], port.decode(jpegs[k])["rgb"].transpose(2, 0, 1))]
print("RESULT", "ok" if not bad else bad[:5])
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-400:] + r.stderr[-400:])
