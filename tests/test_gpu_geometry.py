"""Pictures at the dimension limits on the GPU (run with -m gpu on an MI355X): the family of tests/geometry_corpus.py -- 65535 samples
on one axis, one MCU column thousands of MCU rows tall, MCU grids 8192 wide and 8192 high, 73728 restart segments in one picture, a
DRI of 65535, widths on both sides of 32768 -- on every decode path: lane streams in both plan modes and all three output formats,
each member alone, the exact kernel with the dense back end, picture groups, reduced size, resize on decode (the 64-bit taps, the
top of the 32-bit branch, row taps up to 65534), bound outputs with guard bytes, entropy errors, shards and split decode, the
literal DPU payload, the CLI and the pipelined batcher, and progressive frames.

Every comparison is byte equality, and every expected byte comes from the oracle port (oracle/liboracle.so), tests/resize_model.py,
the box filter of test_gpu_scaled.py or the progressive model of tests/jpeg_progressive.py; none from a decode by this library.  Every
test asserts how many pictures it compared."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import geometry_corpus as G
import jpeg_progressive as P
import progressive_corpus as PC
from conftest import golden_bytes, ROOT
from test_gpu_progressive_streams import expected as progressive_expected, scan_progressive
from test_gpu_resize import expected as resized
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = [(0, 1), (16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)
LANE = [n for n in G.NAMES if n != G.REF_RULE]      # the members the planner takes onto the lane streams
PYTHONPATH = [os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"), HERE]


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(port):
    """name -> the oracle's answer for the member: huff_rc, rgb, bmp, coef, and for the DPU payload test mcus and metadata"""
    G.family()
    out = {}
    for name in G.NAMES:
        o = port.decode(G.oracle_bytes(name))
        assert o["valid"], name
        out[name] = {"huff_rc": o["huff_rc"], "rgb": o["rgb"], "bmp": np.frombuffer(o["bmp"], np.uint8), "coef": o["coef"]}
        if name in DPU_MEMBERS:
            out[name].update(mcus=o["mcus"], metadata=o["metadata"])
    return out


@pytest.fixture(scope="module")
def boxed(oracle):
    """boxed(name, s): the box filter of the oracle's picture, computed once"""
    cache = {}

    def get(name, s):
        if (name, s) not in cache:
            cache[(name, s)] = box(oracle[name]["rgb"], s)
        return cache[(name, s)]
    return get


def _scan(names, extra=0, data_of=G.jpeg):
    import pjd_amd
    out = []
    for n in names:
        s = pjd_amd.Scanned(data_of(n), n + ".jpg")
        assert s.valid, n
        s.desc.flags = int(s.desc.flags) | G.flags(n) | extra
        out.append(s)
    return out


def _fmt(fmt):
    import pjd_amd
    return {"rgb8": pjd_amd.OUT_RGB8, "bmp": pjd_amd.OUT_BMP, "planar": pjd_amd.OUT_RGB8_PLANAR}[fmt]


def bmp_of(rgb):
    import pjd_amd
    return np.frombuffer(pjd_amd.rgb_to_bmp(rgb), np.uint8)


def _same_picture(got, rgb, fmt, label):
    """got, as download() returns it in format fmt, against an H x W x 3 picture"""
    if fmt == "bmp":
        want = bmp_of(rgb)
        got = np.asarray(got).reshape(-1)
        h, w, _ = rgb.shape
        stride = 3 * w + w % 4
        assert got.size == want.size == 26 + h * stride, label
        assert int(got[18]) | int(got[19]) << 8 == w and int(got[20]) | int(got[21]) << 8 == h, label
        assert int.from_bytes(got[2:6].tobytes(), "little") == 26 + h * stride, label
    else:
        want = np.ascontiguousarray(rgb.transpose(2, 0, 1)) if fmt == "planar" else rgb
        assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (label, fmt, "first differing byte", int(bad[0]), "of", got.size, "differing", int(bad.size))


def _same_coefficients(b, k, want, label):
    got = b.coefficients(k)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (label, "coefficients differ from the oracle's at", bad[:4].tolist(), "in", len(bad), "places")


# ---- 1: the whole family in one batch on the lane path ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bmp", "planar"])
@pytest.mark.parametrize("plan_mode", ["latency", "throughput"])
def test_family_in_one_batch_on_the_lane_path(oracle, plan_mode, fmt):
    """Status, picture (whole BMP files with their 16-bit header fields; planes) and, once per plan mode, coefficients of all fifteen
    members; nothing re-decoded, no flagged wave; only the member under the reference's restart rule goes to the exact kernel."""
    import pjd_amd
    c = pjd_amd.Context(0, plan_mode=pjd_amd.PLAN_THROUGHPUT if plan_mode == "throughput" else pjd_amd.PLAN_LATENCY)
    try:
        scanned = _scan(G.NAMES)
        with c.batch([s.desc for s in scanned], _fmt(fmt)) as b:
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
            n = 0
            for k, name in enumerate(G.NAMES):
                assert st[k] == oracle[name]["huff_rc"] == 0, (name, st[k])
                _same_picture(outs[k], oracle[name]["rgb"], fmt, name)
                if fmt == "bmp":
                    assert np.array_equal(np.asarray(outs[k]).reshape(-1), oracle[name]["bmp"]), name
                if fmt == "rgb8":
                    _same_coefficients(b, k, oracle[name]["coef"], name)
                n += 1
        assert n == len(G.NAMES) == 15
        assert info["plan_mode"] == (1 if plan_mode == "throughput" else 0)
        assert info["n_fallback"] == 0 and sum(info["flag_waves"]) == 0 and info["n_sequential"] == 1, info
    finally:
        c.close()


# ---- 2: each member alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_member_alone(ctx, oracle, name):
    """A batch of one: the per-picture subsequence size (the planner's, as pjd_plan_info states it) and the idle-device form of the
    chain see only this picture."""
    import pjd_amd
    s = _scan([name])[0]
    plan = pjd_amd.plan_info([s.desc])
    with ctx.batch([s.desc]) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
        assert st == [oracle[name]["huff_rc"]] == [0], name
        _same_picture(outs[0], oracle[name]["rgb"], "rgb8", name)
        _same_coefficients(b, 0, oracle[name]["coef"], name)
    assert len(outs) == 1
    assert info["sub_bytes"] == plan["sub_bytes"] and info["n_subsequences"] == plan["n_subsequences"], (info, plan)
    assert info["n_fallback"] == 0 and sum(info["flag_waves"]) == 0 and info["n_sequential"] == (name == G.REF_RULE), info


# ---- 3: the exact kernel and the dense back end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_family_through_the_exact_kernel(ctx, oracle, fmt):
    import pjd_amd
    scanned = _scan(G.NAMES, pjd_amd.F_FORCE_SEQUENTIAL)
    with ctx.batch([s.desc for s in scanned], _fmt(fmt)) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
        n = 0
        for k, name in enumerate(G.NAMES):
            assert st[k] == 0, name
            _same_picture(outs[k], oracle[name]["rgb"], fmt, name)
            if fmt == "rgb8":
                _same_coefficients(b, k, oracle[name]["coef"], name)
            n += 1
    assert n == 15 and info["n_sequential"] == len(G.NAMES), info


# ---- 4: picture groups --------------------------------------------------------------------------------------------------------------
def test_picture_groups(ctx, oracle):
    """The lane-path members but the two 65535 x 72 ones, repeated to 64 pictures: the group form of the DC scan."""
    names = [n for n in LANE if n not in G.BIG]
    names = (names * (64 // len(names) + 1))[:64]
    assert len(names) == 64 and len(set(names)) == 12
    scanned = _scan(names)
    with ctx.batch([s.desc for s in scanned]) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    n = 0
    for k, name in enumerate(names):
        assert st[k] == 0, (k, name)
        _same_picture(outs[k], oracle[name]["rgb"], "rgb8", (k, name))
        n += 1
    assert n == 64 and info["n_sequential"] == 0 and info["n_fallback"] == 0, info


# ---- 5: reduced size -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bmp", "planar"])
@pytest.mark.parametrize("mode", ["lanes", "dense"])
def test_family_at_every_scale_beside_the_full_size_twin(ctx, oracle, boxed, mode, fmt):
    """Every member at 1/1, 1/2, 1/4 and 1/8 in one batch.  Width 65535 gives 32768, 16384 and 8192 columns, the last box 1, 3 and 7
    columns wide, and no planar row but the first starts on a multiple of four bytes."""
    import pjd_amd
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "dense" else 0
    rows, scanned = [], []
    for flags, s in SCALES:
        for name, sc in zip(G.NAMES, _scan(G.NAMES, extra | flags)):
            rows.append((name, flags, s))
            scanned.append(sc)
    with ctx.batch([x.desc for x in scanned], _fmt(fmt)) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
    n = 0
    for k, (name, flags, s) in enumerate(rows):
        w, h, _, _ = G.geometry(name)
        want = boxed(name, s)
        assert pjd_amd.scaled_dims(w, h, flags) == (want.shape[1], want.shape[0]) == (-(-w // s), -(-h // s)), (name, s)
        if w == 65535 and s > 1:
            assert want.shape[1] == 65536 // s and w - (want.shape[1] - 1) * s == s - 1, (name, s)      # the last box: s - 1 columns
        assert st[k] == 0, (name, s)
        _same_picture(outs[k], want, fmt, (name, s))
        n += 1
    assert n == 60
    if mode == "dense":
        assert info["n_sequential"] == 60, info
    else:
        assert info["n_fallback"] == 0 and info["n_sequential"] == 4, info      # the `_ref` member at its four scales


# ---- 6: resize on decode ---------------------------------------------------------------------------------------------------------------
RESIZE = [("w65535x8_444", 0, (65535, 1)),                   # 64-bit taps along x at the identity width
          ("w65535x8_444", 0, (1, 1)),
          ("w32768x8_444", 0, (65535, 3)),                   # the 32-bit branch at the top of its range: sn * dn = 2^31 - 32768
          ("w32769x17_440", 0, (65535, 3)),                  # the first width past the branch
          ("h8x65535_444_ri1", 0, (1, 65535)),               # row taps with y0 up to 65534
          ("h8x65535_444_ri1", 0, (3, 32769)),
          ("h1x65535_440", 0, (224, 224)),
          ("w65535x1_grey", 0, (224, 224)),
          ("w65535x1_grey", 0, (65535, 2)),                  # a one-row source upscaled
          ("segs_65535x72_444_ri1", 48, (8192, 9))]          # the identity after the 1/8 pre-scale


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_resize_at_the_dimension_limits(ctx, oracle, boxed, fmt):
    """(tw, th) per descriptor above, in one batch: the model over the oracle's picture (over its 1/8 box for the last one, which it
    must reproduce: the identity target)."""
    planar = fmt == "planar"
    scanned = [_scan([name], flags)[0] for name, flags, _ in RESIZE]
    with ctx.batch([s.desc for s in scanned], _fmt(fmt)) as b:
        b.set_resize([(th, tw) for _, _, (tw, th) in RESIZE])
        b.upload(); b.decode()
        outs, st = b.download()
    n = 0
    for k, (name, flags, (tw, th)) in enumerate(RESIZE):
        s = 1 << (flags >> 4)
        want = resized(oracle[name]["rgb"], s, tw, th, planar)
        assert st[k] == 0, (name, tw, th)
        assert outs[k].shape == want.shape == ((3, th, tw) if planar else (th, tw, 3)), (name, tw, th)
        bad = np.argwhere(outs[k] != want)
        assert bad.size == 0, (name, tw, th, "first differing sample", bad[0].tolist(), "differing", len(bad))
        if name == "segs_65535x72_444_ri1":
            assert np.array_equal(outs[k], boxed(name, 8).transpose(2, 0, 1) if planar else boxed(name, 8))
        n += 1
    assert n == 10


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_resize_targets_around_the_tile_edges(ctx, port, fmt):
    """A tile of the resize kernel is 8 rows x 256 columns (PJD_RS_ROWS, PJD_RS_COLS): targets one under, at and one over one and two
    tiles on both axes, 25 descriptors of one small fixture in one batch."""
    import pjd_amd
    planar = fmt == "planar"
    data = golden_bytes("big_640x480_420_q85")
    rgb = port.decode(data)["rgb"]
    targets = [(tw, th) for tw in (255, 256, 257, 511, 513) for th in (7, 8, 9, 15, 17)]
    scanned = [pjd_amd.Scanned(data) for _ in targets]
    with ctx.batch([s.desc for s in scanned], _fmt(fmt)) as b:
        b.set_resize([(th, tw) for tw, th in targets])
        b.upload(); b.decode()
        outs, st = b.download()
    assert st == [0] * 25
    for (tw, th), o in zip(targets, outs):
        assert np.array_equal(o, resized(rgb, 1, tw, th, planar)), (tw, th)
    assert len(outs) == 25


# ---- 7: guard bytes --------------------------------------------------------------------------------------------------------------------
GUARD = ["w65535x8_444", "h1x65535_440", "w65535x1_grey"]

GUARD_CHILD = """
import torch                                      # first: torch and the library then share one HIP runtime
torch.zeros(1, device="cuda:0"); torch.cuda.synchronize()
import json, sys
sys.path[:0] = json.loads(sys.argv[2])
import numpy as np, pjd_amd
work = sys.argv[1]
items = json.load(open(work + "/items.json"))       # [[file, flags, key of the expected picture]]
want = np.load(work + "/want.npz")
ctx = pjd_amd.Context(0)
n = 0
for fmt in (pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_RGB8):
    scanned = []
    for f, flags, key in items:
        s = pjd_amd.Scanned(open(work + "/" + f, "rb").read())
        assert s.valid
        s.desc.flags = int(s.desc.flags) | flags
        scanned.append(s)
    with ctx.batch([s.desc for s in scanned], fmt) as b:
        offs, pos = [], 1                             # base + 1: no picture starts aligned, and odd gaps between them
        for i in range(b.n):
            offs.append(pos)
            pos += b.output_size(i) + 2 * i + 1
        total = pos + 4096
        buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 4 == 0
        b.bind_output(buf.data_ptr(), total, offs)
        b.upload()
        for phase in ("decode", "replay"):
            if phase == "replay":
                b.capture()
                buf.fill_(0xA5)
                torch.cuda.synchronize()
            b.decode(); b.sync()
            assert b.statuses() == [0] * b.n
            host = buf.cpu().numpy()
            covered = np.zeros(total, bool)
            for i, (f, flags, key) in enumerate(items):
                w = want[key]
                w = np.ascontiguousarray(w.transpose(2, 0, 1)) if fmt == pjd_amd.OUT_RGB8_PLANAR else w
                assert b.output_size(i) == w.size, (f, flags)
                got = host[offs[i]:offs[i] + w.size]
                bad = np.flatnonzero(got != w.reshape(-1))
                assert bad.size == 0, (phase, fmt, f, flags, "first differing byte", int(bad[0]), "differing", int(bad.size))
                covered[offs[i]:offs[i] + w.size] = True
                n += 1
            stray = np.flatnonzero(~covered & (host != 0xA5))
            assert stray.size == 0, (phase, fmt, "bytes outside every picture were written, first at", stray[:8].tolist(), offs)
ctx.close()
print("RESULT ok", n)
"""


def test_bound_outputs_at_base_plus_one_keep_their_guard_bytes(tmp_path, oracle, boxed):
    """Planar and interleaved outputs of three strips at 1/1 and 1/4 bound at base + 1 in a buffer of 0xA5 (torch owns it: a child
    process, torch loaded first): every picture is the oracle's, every other byte still 0xA5; again after capture() and a replay
    over the refilled buffer."""
    items, want = [], {}
    for name in GUARD:
        (tmp_path / (name + ".jpg")).write_bytes(G.jpeg(name))
        for flags, s in ((0, 1), (32, 4)):
            items.append([name + ".jpg", flags, f"{name}:{s}"])
            want[f"{name}:{s}"] = boxed(name, s)
    (tmp_path / "items.json").write_text(json.dumps(items))
    np.savez(tmp_path / "want.npz", **want)
    r = subprocess.run([sys.executable, "-c", GUARD_CHILD, str(tmp_path), json.dumps(PYTHONPATH)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"RESULT ok {2 * 2 * len(items)}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])
    assert len(items) == 6


# ---- 8: entropy errors in strips -------------------------------------------------------------------------------------------------------
CUT = ["w65535x16_420", "h8x65535_444_ri1", "h9x65535_422", "segs_65535x72_444_ri1"]


def test_truncated_strips_keep_status_and_partial_picture(ctx, port, oracle, boxed):
    """Each of four members cut to half of its entropy-coded bytes, beside its intact twin, at full size and at 1/8: the oracle's
    status (an error for every cut), its partial picture (grey behind the error) and its coefficients.

    Nothing is re-decoded (n_fallback == 0), as test_corrupt_and_truncated_4k_pictures_settle_on_the_parallel_path asserts.  That test
    also asserts n_sequential == 0; its picture has no restart markers.  A cut through a picture with DRI takes restart markers away,
    the scanner then finds fewer segments than ceil(n_mcu / DRI), and the planner routes such a picture to the exact kernel up front
    (pjd_plan.cpp: n_segments != nseg_total): that is routing, not a fallback, and it is asserted as such here."""
    import pjd_amd
    cut = {}
    for name in CUT:
        o = port.decode(G.truncated(name))
        assert o["valid"] and o["huff_rc"] != 0, (name, "the cut must leave an entropy-coding error: move it")
        cut[name] = o
    rows, scanned, n_routed = [], [], 0
    for flags, s in (SCALES[0], SCALES[3]):
        for name in CUT:
            for is_cut in (True, False):
                sc = _scan([name], flags, G.truncated if is_cut else G.jpeg)[0]
                if is_cut and G.geometry(name)[3]:
                    assert int(sc.desc.n_segments) < G.n_segments(name), name
                    n_routed += 1
                rows.append((name, s, is_cut))
                scanned.append(sc)
    with ctx.batch([x.desc for x in scanned]) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
        n = 0
        for k, (name, s, is_cut) in enumerate(rows):
            want = cut[name] if is_cut else oracle[name]
            assert st[k] == want["huff_rc"], (name, s, is_cut, st[k])
            _same_picture(outs[k], box(want["rgb"], s) if is_cut else boxed(name, s), "rgb8", (name, s, is_cut))
            if s == 1:
                _same_coefficients(b, k, want["coef"], (name, is_cut))
            n += 1
    assert n == 16 and n_routed == 4
    assert info["n_fallback"] == 0 and info["n_sequential"] == n_routed, info


# ---- 9: shards and split decode ----------------------------------------------------------------------------------------------------------
SPLIT = [("h8x65535_444_ri1", 3), ("segs_65535x72_444_ri1", 8), (G.DRI65535, 2)]


@pytest.mark.parametrize("name,world", SPLIT)
def test_shard_union(ctx, oracle, name, world):
    """Each rank's restart-segment range decoded as a batch of its own from its slice of the stream; the MCUs the ranks own, put
    together, are the oracle's picture."""
    import pjd_amd
    from pjd_amd import parallel
    s = _scan([name])[0]
    segs, ecs, d0 = s.seg_offsets(), s.ecs(), s.desc
    want = oracle[name]["rgb"]
    got = np.zeros_like(want)
    h, w, _ = want.shape
    mcux, ri, n_mcu = (w + 7) // 8, int(d0.restart_interval), G.n_mcu(name)
    mcu_of = (np.arange(h) // 8)[:, None] * mcux + (np.arange(w) // 8)[None, :]
    n_ranks = 0
    for r in range(world):
        f, c = parallel.segment_range(len(segs), r, world)
        assert c > 0
        lo = int(segs[f])
        hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
        d, keep = parallel.shard_descriptor(d0, segs, ecs[lo:hi], lo, r, world)
        outs, st = ctx.decode([d], pjd_amd.OUT_RGB8)
        assert st == [0], (name, r)
        own = (mcu_of >= f * ri) & (mcu_of < min((f + c) * ri, n_mcu))
        got[own] = outs[0][own]
        n_ranks += 1
    assert n_ranks == world
    _same_picture(got, want, "rgb8", name)


@pytest.mark.parametrize("name,world", SPLIT)
def test_split_decode(ctx, oracle, boxed, monkeypatch, name, world):
    """pjd_split_decode with the device listed `world` times, at full size and at 1/2, interleaved and planar: the unsplit decode's
    bytes and the oracle's."""
    import pjd_amd
    monkeypatch.setenv("PJD_PIPE_ALLOW_DUP_DEVICES", "1")
    n = 0
    try:
        for flags, s in SCALES[:2]:
            for fmt in ("rgb8", "planar"):
                sc = _scan([name], flags)[0]
                whole, st = ctx.decode([sc.desc], _fmt(fmt))
                assert st == [0]
                _same_picture(whole[0], boxed(name, s), fmt, (name, s, "unsplit"))
                got, status, stats = pjd_amd.split_decode(sc.desc, [0] * world, _fmt(fmt))
                assert status == 0 and stats["n_ranks"] == min(world, G.n_segments(name)) == world, (name, s, stats)
                assert stats["n_segments"] == G.n_segments(name) and stats["redone_whole"] == 0, (name, s, stats)
                _same_picture(got, boxed(name, s), fmt, (name, s, "split"))
                assert np.array_equal(got, whole[0]), (name, s, fmt)
                n += 1
    finally:
        pjd_amd.dev_lib().pjd_split_release()
    assert n == 4


# ---- 10: the literal DPU payload -----------------------------------------------------------------------------------------------------------
DPU_MEMBERS = ["w65535x16_420", "h1x65535_440", "w65535x1_grey"]


@pytest.mark.parametrize("name", DPU_MEMBERS)
def test_dpu_payload(ctx, oracle, name):
    o = oracle[name]
    n = o["coef"].shape[0]
    mcus = o["coef"].copy()
    ctx.exec_dpu_payload(np.tile(o["metadata"], (n, 1)), mcus)
    assert n == 164 and np.array_equal(mcus, o["mcus"]), name


# ---- 11: the CLI and the pipelined batcher -------------------------------------------------------------------------------------------------
def test_cli_plain_pipelined_and_scaled(tmp_path, oracle, boxed):
    names = ["w65535x8_444", "h8x65535_444_ri1"]
    exe = os.path.join(ROOT, "bin", "decoder")
    n = 0
    for label, extra, s in (("plain", [], 1), ("pipe", ["--pipeline"], 1), ("scaled", ["--scale", "1/8"], 8)):
        d = tmp_path / label
        d.mkdir()
        for name in names:
            (d / (name + ".jpg")).write_bytes(G.jpeg(name))
        p = subprocess.run([exe] + extra + [str(d / (name + ".jpg")) for name in names], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        for name in names:
            got = np.frombuffer((d / (name + ".bmp")).read_bytes(), np.uint8)
            want = oracle[name]["bmp"] if s == 1 else bmp_of(boxed(name, s))
            assert np.array_equal(got, want), (label, name)
            n += 1
    assert n == 6


def test_family_through_the_pipelined_batcher(port, oracle):
    """Batches of four on two slots.  The batcher gives every picture the same flags, so the `_std` member is decoded under the
    reference's restart rule like its `_ref` twin: the expected file is the oracle's BMP of the member's own bytes."""
    import pjd_amd
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            assert index not in got
            got[index] = (name, status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=[G.jpeg(n) for n in G.NAMES], names=[n + ".jpg" for n in G.NAMES], out_format=pjd_amd.OUT_BMP,
                          batch_images=4, slots=2, sink=sink)
    assert st["n_decoded"] == 15 and st["n_batches"] == 4 and st["n_batch_failures"] == 0 and st["n_rejected"] == 0, st
    assert G.jpeg(G.STD_RULE) == G.jpeg(G.REF_RULE)
    for k, name in enumerate(G.NAMES):
        want = oracle[G.REF_RULE if name == G.STD_RULE else name]
        assert got[k][0] == name + ".jpg" and got[k][1] == want["huff_rc"], name
        assert np.array_equal(got[k][2], want["bmp"]), name
    assert len(got) == 15
    assert st["out_bytes"] == sum(len(oracle[G.REF_RULE if n == G.STD_RULE else n]["bmp"]) for n in G.NAMES)


# ---- 12: progressive frames --------------------------------------------------------------------------------------------------------------------
# (label, sampling, w, h, PC.full_script?)  The full dimension with a short script (DC first at Al = 0, then one AC band 1..63), a quarter
# of it with every refinement level: the writer and the model take some ten seconds of CPU per frame at 65521 x 16 and 9 x 65535.
# full_script's luma AC scans are not interleaved and cover ceil(w / 8) block columns: 2047 of the 2048 of the MCU grid at 16369.
PROGRESSIVE = [("grey_65535x8", "grey", 65535, 8, False), ("grey_8x65535", "grey", 8, 65535, False),
               ("420_16377x16", "420", 16377, 16, True), ("422_9x16383", "422", 9, 16383, True), ("420_16369x16", "420", 16369, 16, True)]


@pytest.fixture(scope="module")
def progressive(port):
    """[(label, data, frame, (status, coefficients, rgb) of the model)]"""
    rng = np.random.default_rng(65535)
    out = []
    for label, sub, w, h, full in PROGRESSIVE:
        fr = PC.frame_of(sub, w, h)
        if full:
            wr = P.build(fr, PC.random_target(fr, rng), PC.full_script(fr))
        else:       # one band at Al = 0: magnitudes to 255, so that the band's table stays within the 162 symbols a table holds
            wr = P.build(fr, PC.random_target(fr, rng, amp=255), [P.S(0, al=0), P.S(0, 1, 63, 0, 0)])
        out.append((label, wr.data, fr, progressive_expected(port, wr.data, fr)))
    return out


@pytest.mark.parametrize("k", range(len(PROGRESSIVE)), ids=[p[0] for p in PROGRESSIVE])
def test_progressive_frame_alone_and_at_quarter_size(ctx, progressive, k):
    """Status, coefficients and picture of the T.81 model (tests/jpeg_progressive.py) through the oracle port's back end, as
    test_gpu_progressive_streams.py compares; at 1/4 the box filter of the model's picture."""
    import pjd_amd
    label, data, fr, (status, coef, rgb) = progressive[k]
    assert status == 0 and rgb.shape == (fr.height, fr.width, 3), label
    s = scan_progressive(data)
    with ctx.batch([s.desc]) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        assert st == [0], label
        _same_coefficients(b, 0, coef, label)
        _same_picture(outs[0], rgb, "rgb8", label)
    q = scan_progressive(data, pjd_amd.F_SCALE_1_4)
    outs4, st = ctx.decode([q.desc], pjd_amd.OUT_RGB8)
    assert st == [0], label
    _same_picture(outs4[0], box(rgb, 4), "rgb8", (label, "1/4"))
    assert len(outs) + len(outs4) == 2
