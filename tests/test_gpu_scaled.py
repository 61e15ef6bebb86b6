"""Reduced-size output on the GPU (run with -m gpu on an MI355X): PJD_F_SCALE_1_2 / _1_4 / _1_8 through every layer -- batch back
ends (lane streams, picture groups, exact kernel, progressive frames), shards, split decode, pipelined batcher, CLI.  The expected
picture is always a numpy box filter (include/pjd.h: rounded mean of the clamped 8-bit colours of each s x s box, cut at the right and
bottom edge) over the oracle's picture, or over this library's own full-size picture where no oracle exists (progressive frames)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_bytes, ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
HUFF_ERR = sorted(k for k in VALID if MANIFEST[k]["huff_ok"] == 0)
SCALES = [(16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)


def box(rgb, s):
    """H x W x 3 uint8 -> ceil(H/s) x ceil(W/s) x 3: (sum + n/2) // n over each box of the picture."""
    if s == 1:
        return rgb
    h, w, _ = rgb.shape
    sh, sw = -(-h // s), -(-w // s)
    acc = np.zeros((sh * s, sw * s, 3), np.int64)
    acc[:h, :w] = rgb
    cnt = np.zeros((sh * s, sw * s), np.int64)
    cnt[:h, :w] = 1
    tot = acc.reshape(sh, s, sw, s, 3).sum(axis=(1, 3))
    n = cnt.reshape(sh, s, sw, s).sum(axis=(1, 3))[..., None]
    return ((tot + (n >> 1)) // n).astype(np.uint8)


def bmp_of(rgb):
    import pjd_amd
    return np.frombuffer(pjd_amd.rgb_to_bmp(rgb), np.uint8)


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


def _scanned(data, flags):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _check(names, outs, st, want_of, fmt):
    import pjd_amd
    for (n, s), o, status in zip(names, outs, st):
        want_st, want_rgb = want_of(n)
        assert status == want_st, (n, s)
        want = box(want_rgb, s)
        if fmt == pjd_amd.OUT_BMP:
            assert np.array_equal(np.asarray(o).reshape(-1), bmp_of(want)), (n, s)
        else:
            assert o.shape == want.shape and np.array_equal(o, want), (n, s, o.shape, want.shape)


# ---- 1-3: every fixture, one mixed-scale batch, both back ends ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("fmt", ["rgb8", "bmp"])
def test_fixtures_mixed_scale_batch_match_box_of_oracle(ctx, oracle, mode, fmt):
    """All decodable fixtures (every sampling mode, grey, odd sizes, wrap_*, restart intervals, div_rst_* garble, entropy errors) at
    s = 1, 2, 4 and 8 in ONE batch: byte equality with the box filter of the oracle's picture (whole BMP files: header, rows,
    padding); the full-size members of the batch stay the oracle's pictures."""
    import pjd_amd
    out_fmt = pjd_amd.OUT_BMP if fmt == "bmp" else pjd_amd.OUT_RGB8
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    names, scanned = [], []
    for n in VALID:
        for flags, s in [(0, 1)] + SCALES:
            names.append((n, s))
            scanned.append(_scanned(golden_bytes(n), flags | extra))
    with ctx.batch([x.desc for x in scanned], out_fmt) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    if mode == "exact":
        assert info["n_sequential"] == len(scanned)
    _check(names, outs, st, lambda n: oracle[n], out_fmt)
    want_bytes = sum(int(pjd_amd.image_output_size(x.desc, out_fmt)) for x in scanned)
    assert info["out_bytes"] == want_bytes
    assert info["pixels"] == sum(int(x.desc.width) * int(x.desc.height) for x in scanned)


def test_entropy_error_fixtures_keep_status_and_partial_picture(ctx, oracle):
    """huff_ok == 0 fixtures (corrupt, truncated, huff_longtail_*): the status of s = 1 and the box of the partial picture."""
    import pjd_amd
    assert HUFF_ERR
    for n in HUFF_ERR:
        sc = _scanned(golden_bytes(n), 0)                    # the descriptor lives as long as its Scanned
        full, st1 = ctx.decode([sc.desc], pjd_amd.OUT_RGB8)
        assert st1[0] == oracle[n][0] != 0, n
        for flags, s in SCALES:
            sc = _scanned(golden_bytes(n), flags)
            outs, st = ctx.decode([sc.desc], pjd_amd.OUT_RGB8)
            assert st == st1, (n, s)
            assert np.array_equal(outs[0], box(oracle[n][1], s)), (n, s)


# ---- 4: a cfg3-style batch ----------------------------------------------------------------------------------------------------
def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


@pytest.mark.parametrize("plan_mode", [0, 1])
def test_cfg3_batch_round_robin_scales(port, plan_mode):
    """1024 ImageNet-like pictures with the scales 1, 1/2, 1/4, 1/8 assigned round-robin: box of the same library's full-size
    decode (and of the oracle on a sample), graph capture + replay idempotent, packed download equal, same fallbacks as s = 1."""
    import pjd_amd
    synth = _synth()
    jpegs = synth.cfg3_imagenet_like(1024, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    c = pjd_amd.Context(0, plan_mode=plan_mode)
    try:
        full_sc = [_scanned(j, 0) for j in jpegs]
        with c.batch([x.desc for x in full_sc]) as b:
            b.upload(); b.decode()
            full, st_full = b.download()
            fb_full = b.info()["n_fallback"]
        scales = [1, 2, 4, 8]
        flag_of = {1: 0, 2: 16, 4: 32, 8: 48}
        sc = [_scanned(j, flag_of[scales[i % 4]]) for i, j in enumerate(jpegs)]
        with c.batch([x.desc for x in sc]) as b:
            b.upload(); b.capture()
            b.decode()
            outs, st = b.download()
            info = b.info()
            b.decode(); b.decode()
            outs2, st2 = b.download()
            packed, st3 = b.download_packed()
        assert st == st_full and st2 == st and st3 == st
        assert info["n_fallback"] == fb_full and info["plan_mode"] == plan_mode
        for i in range(1024):
            want = box(full[i], scales[i % 4])
            assert np.array_equal(outs[i], want), i
            assert np.array_equal(outs2[i], want), i
            assert np.array_equal(packed[i], want.reshape(-1)), i
        for i in (0, 1, 2, 3, 513, 1022):
            assert np.array_equal(outs[i], box(port.decode(jpegs[i])["rgb"], scales[i % 4])), i
    finally:
        c.close()


def test_scaled_batch_of_80_replayed_on_an_idle_device():
    """A batch of 80 pictures at all four scales, captured and replayed on an idle device (a child process of its own: nothing else
    of this suite is on the device): it takes the picture groups and comes out right."""
    code = f"""
import os, sys
sys.path.insert(0, {os.path.join(ROOT, "pim-jpeg-decoder_amd", "python")!r}); sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.join(ROOT, "tools")!r})
import numpy as np, pjd_amd, oracle_lib, synth
from test_gpu_scaled import box
port = oracle_lib.Port()
jpegs = synth.cfg3_imagenet_like(80, seed=31, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
sc = [pjd_amd.Scanned(j) for j in jpegs]
for k, s in enumerate(sc): s.desc.flags = [0, 16, 32, 48][k % 4]
ctx = pjd_amd.Context(0)
b = ctx.batch([s.desc for s in sc], pjd_amd.OUT_RGB8)
b.upload(); b.capture()
for rep in range(2):
    b.decode(); b.sync()
    assert b.decode_chains() == 3, (rep, b.decode_chains())
outs, st = b.download()
bad = [k for k in range(len(jpegs)) if st[k] != 0 or not np.array_equal(outs[k], box(port.decode(jpegs[k])["rgb"], [1, 2, 4, 8][k % 4]))]
print("RESULT", "ok" if not bad else bad[:5])
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-400:] + r.stderr[-400:])


# ---- 5: shards and split decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", [("rstrow_200x150_444_opt", 2), ("rst4_128x96_444", 4), ("rstrow_gray_100x60", 3)])
def test_shard_unions_at_every_scale(ctx, oracle, name, world):
    """Restart-segment shards (shard_first_seg / shard_n_segs) write whole MCUs of the scaled picture: their union is the box of
    the oracle's picture.  rst4_128x96_444 has 16 MCUs per row and RI 4: shard boundaries inside MCU rows."""
    import pjd_amd
    from pjd_amd import parallel
    for flags, s in SCALES:
        sc = _scanned(golden_bytes(name), flags)
        segs, ecs = sc.seg_offsets(), sc.ecs()
        d0 = sc.desc
        want = box(oracle[name][1], s)
        got = np.zeros_like(want)
        mcux = (d0.width + 7) // 8
        m = 8 // s                                                    # 1x1 luma: an MCU is 8 x 8 source pixels
        for r in range(world):
            f, c = parallel.segment_range(len(segs), r, world)
            lo = int(segs[f])
            hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
            d, keep = parallel.shard_descriptor(d0, segs, ecs[lo:hi], lo, r, world)
            outs, st = ctx.decode([d], pjd_amd.OUT_RGB8)
            assert st == [0] and outs[0].shape == want.shape
            m0, m1 = f * d0.restart_interval, min((f + c) * d0.restart_interval, mcux * ((d0.height + 7) // 8))
            for k in range(m0, m1):
                y0, x0 = (k // mcux) * m, (k % mcux) * m
                got[y0:y0 + m, x0:x0 + m] = outs[0][y0:y0 + m, x0:x0 + m]
        assert np.array_equal(got, want), (name, s)


@pytest.mark.parametrize("fmt", ["bmp", "rgb8"])
def test_split_decode_at_every_scale_equals_batch_path(ctx, monkeypatch, fmt):
    """pjd_split_decode with the device listed 1, 2, 3 and 5 times: the same bytes as the one-device batch decode at every scale,
    also where a range boundary falls inside an MCU row and for 4:2:0 under the standard restart rule."""
    import pjd_amd
    monkeypatch.setenv("PJD_PIPE_ALLOW_DUP_DEVICES", "1")
    synth = _synth()
    out_fmt = pjd_amd.OUT_BMP if fmt == "bmp" else pjd_amd.OUT_RGB8
    cases = [("rstrow_200x150_444_opt", golden_bytes("rstrow_200x150_444_opt"), 0),
             ("rst4_128x96_444", golden_bytes("rst4_128x96_444"), 0),
             ("rstrow_gray_100x60", golden_bytes("rstrow_gray_100x60"), 0),
             ("1000x700 4:2:0 RI 7 standard rule", synth.make(1000, 700, 77, 90, synth.SUB_420, 7, synth.DENSE_DETAIL, True),
              pjd_amd.F_STANDARD_RESTART)]
    for label, data, extra in cases:
        for flags, s in SCALES:
            sc = _scanned(data, flags | extra)
            whole, st = ctx.decode([sc.desc], out_fmt)
            assert st == [0]
            sc1 = _scanned(data, extra)
            full, _ = ctx.decode([sc1.desc], pjd_amd.OUT_RGB8)
            want = box(full[0], s)
            ref = bmp_of(want) if out_fmt == pjd_amd.OUT_BMP else want.reshape(-1)
            assert np.array_equal(np.asarray(whole[0]).reshape(-1), ref), (label, s)
            for world in (1, 2, 3, 5):
                got, status, stats = pjd_amd.split_decode(sc.desc, [0] * world, out_fmt)
                assert status == 0 and stats["redone_whole"] == 0, (label, s, world)
                assert stats["n_ranks"] == min(world, int(sc.desc.n_segments)), (label, s, world, stats)
                assert np.array_equal(np.asarray(got).reshape(-1), ref), (label, s, world)
    pjd_amd.dev_lib().pjd_split_release()


# ---- 6-7: progressive frames, coefficients ------------------------------------------------------------------------------------
def test_progressive_quarter_scale_is_the_box_of_its_full_picture(ctx):
    import io
    PIL = pytest.importorskip("PIL.Image")
    import pjd_amd
    rng = np.random.default_rng(5)
    for (w, h, sub) in [(101, 77, 2), (64, 48, 0), (33, 70, 1)]:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([127 + 100 * np.sin(xx / 9.0), 127 + 90 * np.cos(yy / 17.0), (xx + yy) * 255 / (w + h)], -1) + rng.normal(0, 12, (h, w, 3))
        bio = io.BytesIO()
        PIL.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(bio, "JPEG", quality=85, subsampling=sub, progressive=True)
        descs = []
        for flags in (0, pjd_amd.F_SCALE_1_4):
            s = pjd_amd.Scanned(bio.getvalue(), options=pjd_amd.SCAN_PROGRESSIVE)
            assert s.valid and int(s.desc.n_scans) >= 2
            s.desc.flags = int(s.desc.flags) | flags
            descs.append(s)
        with ctx.batch([x.desc for x in descs]) as b:
            b.upload(); b.decode()
            outs, st = b.download()
        assert st == [0, 0]
        assert np.array_equal(outs[1], box(outs[0], 4)), (w, h, sub)


def test_coefficients_do_not_depend_on_the_scale(ctx):
    import pjd_amd
    names = ["ilsvrc_val_00000001", "big_640x480_420_q85", "rst4_128x96_444", "gray_61x45"]
    for extra in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        sc = [_scanned(golden_bytes(n), flags | extra) for n in names for flags in (0, 16, 32, 48)]
        with ctx.batch([x.desc for x in sc]) as b:
            b.upload(); b.decode()
            b.download()
            for k in range(len(names)):
                c0 = b.coefficients(4 * k)
                for j in (1, 2, 3):
                    assert np.array_equal(b.coefficients(4 * k + j), c0), (names[k], j)
                assert hashlib.sha256(c0.tobytes()).hexdigest() == MANIFEST[names[k]]["coef_sha256"], names[k]


# ---- 8: pipelined batcher ---------------------------------------------------------------------------------------------------
def test_pipeline_image_flags_half_scale(ctx, oracle):
    import threading
    import pjd_amd
    names = sorted(MANIFEST)
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            got[index] = (status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=[golden_bytes(n) for n in names], names=[n + ".jpg" for n in names], out_format=pjd_amd.OUT_BMP,
                          batch_images=7, slots=2, sink=sink, image_flags=pjd_amd.F_SCALE_1_2)
    assert st["n_decoded"] == len(VALID) and st["n_batch_failures"] == 0
    total = 0
    for i, n in enumerate(names):
        status, data = got[i]
        if MANIFEST[n]["rc"] != 0:
            assert status == -1 and data is None, n
            continue
        assert status == oracle[n][0], n
        want = bmp_of(box(oracle[n][1], 2))
        assert np.array_equal(data, want), n
        total += len(want)
    assert st["out_bytes"] == total
    assert st["pixels"] == sum(MANIFEST[n]["dims"][0] * MANIFEST[n]["dims"][1] for n in VALID)


# ---- 9: the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_scale_option(tmp_path, oracle):
    import shutil
    names = ["ilsvrc_val_00000001", "env_61x45_420_q100_opt", "err_truncated_eoi_444", "div_rst_420_64x48", "neg_progressive_64x48"]
    names = [n for n in names if n in MANIFEST]
    exe = os.path.join(ROOT, "bin", "decoder")
    for extra in ([], ["--pipeline"]):
        d = tmp_path / ("pipe" if extra else "plain")
        d.mkdir()
        for n in names:
            shutil.copy(os.path.join(HERE, "golden", n + ".jpg"), d / (n + ".jpg"))
        p = subprocess.run([exe, "--scale", "1/4"] + extra + [str(d / (n + ".jpg")) for n in names], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        for n in names:
            bmp = d / (n + ".bmp")
            if MANIFEST[n]["rc"] != 0:
                assert not bmp.exists(), n
            else:
                assert np.array_equal(np.frombuffer(bmp.read_bytes(), np.uint8), bmp_of(box(oracle[n][1], 4))), (n, extra)
    bad = tmp_path / "bad"
    bad.mkdir()
    shutil.copy(os.path.join(HERE, "golden", "ilsvrc_val_00000001.jpg"), bad / "a.jpg")
    q = subprocess.run([exe, "--scale", "3/4", str(bad / "a.jpg")], capture_output=True, text=True, timeout=120)
    assert q.returncode != 0 and not (bad / "a.bmp").exists()
    q = subprocess.run([exe, "--scale", "1/1", str(bad / "a.jpg")], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and hashlib.sha256((bad / "a.bmp").read_bytes()).hexdigest() == MANIFEST["ilsvrc_val_00000001"]["bmp_sha256"]
