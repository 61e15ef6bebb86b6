"""PJD_F_LIBJPEG on the GPU beyond its 136 x 72 fixtures (run with -m gpu on an MI355X): the seeded family of tests/libjpeg_corpus.py --
every width and height from 1 x 1 to 20 x 9 in the four samplings, tile-edge widths, restart markers, saturating content, strips
65500 and 65535 samples long -- on the lane path in both plan modes and with 128-byte lanes, through the exact kernel, in batches
large enough for the planner's picture groups, captured and replayed, on poisoned memory, with bound output, through the
exact-kernel fallback of settle() with the resize and pad launches behind it, cut short at 20, 50 and 90 %, and through bin/decoder
--libjpeg and the pipelined batcher.

Every comparison is byte equality with libjpeg_corpus.expected(port, ...): tests/libjpeg_model.py over the oracle port's
coefficients, which tests/test_libjpeg_corpus_cpu.py holds equal to Pillow's decode wherever libjpeg decodes the file.  Nothing
expected is something this library delivered, and nothing here reads Pillow."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import libjpeg_corpus as LC
import resize_pad_model as pm
from conftest import golden_bytes, ROOT
from test_gpu_poisoned_memory import _fmt, _misplaced_restart_markers, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(ROOT, "bin", "decoder")
LONG = [n for n, _ in LC.limits()]
CUT_MEMBERS = ["e259x37_420", "e515x21_422", LC.WIDE_420]
CUTS = [0.2, 0.5, 0.9]


@functools.lru_cache(maxsize=1)
def _port():
    import oracle_lib
    return oracle_lib.Port()


@functools.lru_cache(maxsize=None)
def _expected_of(data):
    status, rgb = LC.expected(_port(), data)
    rgb.setflags(write=False)
    return status, rgb


def want(name):
    """(status, picture) of the flagged member"""
    return _expected_of(LC.model_bytes(name))


@functools.lru_cache(maxsize=None)
def _reference_picture(data):
    o = _port().decode(data)
    o["rgb"].setflags(write=False)
    return o["huff_rc"], o["rgb"]


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


def scan(data, flagged=True, extra=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid, s.log
    s.desc.flags = int(s.desc.flags) | (pjd_amd.F_LIBJPEG if flagged else 0) | extra
    return s


def decode_and_check(c, rows, fmt="rgb8", decodes=1, capture=False):
    """rows: [(label, scanned, status, picture)].  -> (info, the downloaded pictures)"""
    with c.batch([s.desc for _, s, _, _ in rows], _fmt(fmt)) as b:
        b.upload()
        if capture:
            b.decode(); b.sync()
            b.capture()
        for rep in range(decodes):
            b.decode(); b.sync()
            outs, st = b.download()
            for k, (label, _, status, rgb) in enumerate(rows):
                assert st[k] == status, (label, rep, st[k], status)
                _same(outs[k], rgb, fmt, (label, rep))
        info = b.info()
    assert len(outs) == len(rows)
    return info, outs


@functools.lru_cache(maxsize=None)
def _small_rows_data(tag):
    """The 180 pictures of one sampling flagged, interleaved one for one with the same 180 unflagged: [(label, data, flagged, status,
    picture)], the unflagged ones with the oracle port's (the reference's) picture."""
    rows = []
    for name, data in LC.small(tag):
        rows.append((name, data, True) + want(name))
        rows.append((name + ":plain", data, False) + _reference_picture(data))
    assert len(rows) == 360 and all(r[3] == 0 for r in rows)
    return tuple(rows)


def small_rows(tag, extra_on_flagged=0):
    return [(label, scan(data, flagged, extra_on_flagged if flagged else 0), st, rgb) for label, data, flagged, st, rgb in _small_rows_data(tag)]


# ---- 1: the small family, 360 pictures a batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "planar", "bmp"])
@pytest.mark.parametrize("tag", list(LC.SAMPLINGS))
def test_small_family_in_one_batch(ctx, tag, fmt):
    """Flagged and unflagged twins of all 180 sizes in one batch of 360: the planner builds picture groups and the libjpeg branch
    clears them; nothing is re-decoded and nothing goes to the exact kernel."""
    info, _ = decode_and_check(ctx, small_rows(tag), fmt)
    assert info["n_fallback"] == 0 and info["n_sequential"] == 0, info


def test_small_420_batch_under_the_throughput_plan():
    import pjd_amd
    c = pjd_amd.Context(0, plan_mode=pjd_amd.PLAN_THROUGHPUT)
    try:
        info, _ = decode_and_check(c, small_rows("420"))
        assert info["plan_mode"] == 1 and info["n_fallback"] == 0 and info["n_sequential"] == 0, info
    finally:
        c.close()


def test_small_420_batch_with_128_byte_lanes(monkeypatch):
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    c = pjd_amd.Context(0)
    try:
        info, _ = decode_and_check(c, small_rows("420") + edge_rows())
        assert info["sub_bytes"] == 128 and info["n_fallback"] == 0 and info["n_sequential"] == 0, info
    finally:
        c.close()


def test_small_420_batch_with_the_flagged_pictures_forced_to_the_exact_kernel(ctx):
    import pjd_amd
    info, _ = decode_and_check(ctx, small_rows("420", pjd_amd.F_FORCE_SEQUENTIAL))
    assert info["n_sequential"] == 180 and info["n_fallback"] == 0, info


def test_small_420_batch_captured_and_replayed_twice(ctx):
    info, _ = decode_and_check(ctx, small_rows("420"), "planar", decodes=2, capture=True)
    assert info["n_fallback"] == 0 and info["n_sequential"] == 0, info


# ---- 2: edges() and limits() -----------------------------------------------------------------------------------------------------------
def member_rows(names, extra=0):
    return [(n, scan(LC.jpeg(n), True, extra)) + want(n) for n in names]


def edge_rows(extra=0):
    return member_rows([n for n, _ in LC.edges()], extra)


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
@pytest.mark.parametrize("path", ["lanes", "exact"])
@pytest.mark.parametrize("family", ["edges", "limits"])
def test_edges_and_limits_in_one_batch(ctx, family, path, fmt):
    import pjd_amd
    names = [n for n, _ in (LC.edges() if family == "edges" else LC.limits())]
    rows = member_rows(names, pjd_amd.F_FORCE_SEQUENTIAL if path == "exact" else 0)
    assert all(r[2] == 0 for r in rows) and len(rows) == (16 if family == "edges" else 17)
    info, _ = decode_and_check(ctx, rows, fmt)
    assert info["n_fallback"] == 0 and info["n_sequential"] == (len(rows) if path == "exact" else 0), info


@pytest.mark.parametrize("name", LONG)
def test_long_member_alone(ctx, name):
    """A batch of one: the planner's per-picture choices and the colour launch's workgroup list see only this picture."""
    info, _ = decode_and_check(ctx, member_rows([name]))
    assert info["n_fallback"] == 0 and info["n_sequential"] == 0, info


def _torch_case(case, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "libjpeg_corpus_torch_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_wide_member_bound_at_base_plus_one_keeps_its_guard_bytes():
    """The 65535-wide 4:2:0 member, planar and interleaved, bound at base + 1 in a buffer of 0xA5 that torch owns (a child process,
    torch loaded first): the picture is the model's and every byte before and behind it still 0xA5."""
    _torch_case("bound_output_wide")


# ---- 3: the fallback branch of settle() ------------------------------------------------------------------------------------------------
GOOD_BESIDE = ["e259x37_420", "s20x9_422"]


@pytest.fixture
def fresh_poisoned_ctx(monkeypatch):
    """A context of its own whose allocations start as 0xA5: the buffer pool of the module's context hands a batch the planes and
    pictures an earlier batch of the same shape left there, and a launch that settle() forgot would go unseen behind them."""
    import pjd_amd
    monkeypatch.setenv("PJD_DEBUG_POISON", "0xa5")
    c = pjd_amd.Context(0)
    yield c
    c.close()


def _fallback_rows(flag_the_broken):
    broken = list(_misplaced_restart_markers())
    assert len(broken) >= 6
    rows = []
    if flag_the_broken:
        rows += [(f"broken{k}:flagged", scan(j)) + _expected_of(j) for k, j in enumerate(broken)]
    rows += member_rows(GOOD_BESIDE)
    rows += [(f"broken{k}:plain", scan(j, False)) + _reference_picture(j) for k, j in enumerate(broken)]
    return rows


def test_fallback_redecodes_flagged_pictures(fresh_poisoned_ctx):
    """Restart markers a byte off (4:4:4 and grey: the reference's restart rule is T.81's): the parallel decoder flags the pictures and
    settle() decodes them again with the exact kernel -- for the flagged ones through the dense libjpeg IDCT and the colour launch a
    second time.  More pictures are re-decoded than in the same batch without the flagged broken streams: a flagged one is among them."""
    import pjd_amd
    ctx = fresh_poisoned_ctx
    base = _fallback_rows(False)
    assert all(pjd_amd.plan_info([s.desc])["n_sequential"] == 0 for _, s, _, _ in base), "only the decoder can flag them"
    info0, _ = decode_and_check(ctx, base, decodes=2)
    rows = _fallback_rows(True)
    assert any(r[2] != 0 for r in rows if r[0].endswith(":flagged"))
    info, _ = decode_and_check(ctx, rows, decodes=2)
    assert info["n_sequential"] == 0 and info0["n_sequential"] == 0
    assert info["n_fallback"] >= 2 and info["n_fallback"] > info0["n_fallback"] >= 1, (info["n_fallback"], info0["n_fallback"])
    info_p, _ = decode_and_check(ctx, rows, "planar")
    assert info_p["n_fallback"] == info["n_fallback"]


def test_fallback_with_resize_and_pad_behind_it(fresh_poisoned_ctx):
    """The same batch resampled to 40 x 24 with the antialiased filter, one sample of border on every side: settle() issues the resize
    and border launches again behind the re-decode, and they read the libjpeg picture of the second colour launch."""
    import pjd_amd
    ctx = fresh_poisoned_ctx
    rows = _fallback_rows(True)
    pad, fill = (1, 1, 1, 1), (7, 130, 251)
    with ctx.batch([s.desc for _, s, _, _ in rows]) as b:
        b.set_resize([(24, 40)] * len(rows))
        b.set_resize_pad([pad] * len(rows), fill)
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload()
        for rep in range(2):
            b.decode(); b.sync()
            outs, st = b.download()
            for k, (label, _, status, rgb) in enumerate(rows):
                assert st[k] == status, (label, rep)
                _same(outs[k], pm.padded(rgb, None, 40, 24, pad, fill, 1, "antialias"), "rgb8", (label, rep))
        info = b.info()
    assert info["n_fallback"] >= 2, info


# ---- 4: partial pictures -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cut(name, fraction):
    """(data, status, picture) of the member cut to `fraction` of its entropy-coded bytes; the cut is not empty: the picture starts
    decoded and ends grey, and where the cut leaves a whole MCU row behind the one it lies in, that row is grey from its third pixel
    row on (fancy upsampling leans one chroma row up)."""
    assert LC.model_bytes(name) == LC.jpeg(name)
    data = LC.entropy_cut(LC.jpeg(name), fraction)
    status, rgb = _expected_of(data)
    assert status != 0, (name, fraction, "the cut must leave an entropy-coding error")
    w, h, sub = LC.dims(name)
    mh = 8 * LC.LUMA[sub][1]
    assert not (rgb[:8, :8] == 128).all(), (name, fraction, "nothing decoded")
    assert (rgb[-4:, -4:] == 128).all(), (name, fraction, "nothing left grey")
    grey_rows = [r for r in range(-(-h // mh)) if (rgb[r * mh + 2:(r + 1) * mh] == 128).all()]
    decoded_rows = [r for r in range(-(-h // mh)) if not (rgb[r * mh:(r + 1) * mh] == 128).all()]
    assert decoded_rows, (name, fraction)
    if h > mh and fraction <= 0.5:
        assert grey_rows and grey_rows[-1] == -(-h // mh) - 1, (name, fraction, grey_rows)
    return data, status, rgb


@pytest.mark.parametrize("path", ["lanes", "exact"])
def test_partial_pictures(ctx, path):
    """The status is the oracle port's and the picture the model over the PORT'S coefficients (zero behind the error)."""
    import pjd_amd
    rows = []
    for name in CUT_MEMBERS:
        for f in CUTS:
            data, status, rgb = _cut(name, f)
            rows.append((f"{name}@{f}", scan(data, True, pjd_amd.F_FORCE_SEQUENTIAL if path == "exact" else 0), status, rgb))
        rows.append((name,) + member_rows([name])[0][1:])
    assert len(rows) == 12
    info, _ = decode_and_check(ctx, rows)
    assert info["n_fallback"] == 0 and info["n_sequential"] == (9 if path == "exact" else 0), info


# ---- 5: poison ----------------------------------------------------------------------------------------------------------------------------
def test_poisoned_memory_changes_nothing(ctx, monkeypatch):
    import pjd_amd
    rows = small_rows("420") + member_rows([LC.WIDE_420])
    _, plain = decode_and_check(ctx, rows, decodes=2)
    monkeypatch.setenv("PJD_DEBUG_POISON", "0xa5")
    c = pjd_amd.Context(0)
    try:
        _, poisoned = decode_and_check(c, rows, decodes=2)
    finally:
        c.close()
    assert all(np.array_equal(a, b) for a, b in zip(plain, poisoned))


# ---- 6: the CLI and the batcher -----------------------------------------------------------------------------------------------------------
CLI_NAMES = ["e259x37_420", "e515x21_422", "e1030x9_444", "e257x19_grey", "e200x150_444_ri25", "e6x3_420", "e7x2_420", "e10x1_420", "e6x1_422",
             "e11x2_422", "sat67x35_420_q100", "sat67x35_444_q30", "sat259x19_422_q10", "sat130x40_420_q5", "s5x4_420", "s6x9_422",
             "s19x7_420", "s18x9_422", "s13x3_444", "s20x9_grey"]
PIPE_NAMES = CLI_NAMES + ["e2049x17_420", "e301x203_420_q30", "s1x1_420", "s2x9_422", "s3x5_420", "s4x9_422", "s9x2_420", "s15x8_444", "s17x9_420",
                          "s14x1_422"]


def _bmp(rgb):
    import pjd_amd
    return np.frombuffer(pjd_amd.rgb_to_bmp(rgb), np.uint8)


def _all_with_good_status(names):
    assert all(want(n)[0] == 0 for n in names)


@pytest.mark.parametrize("mode", ["plain", "pipeline"])
def test_cli_libjpeg(tmp_path, mode):
    assert len(CLI_NAMES) == 20 and {LC.dims(n)[0] % 4 for n in CLI_NAMES} == {0, 1, 2, 3}
    _all_with_good_status(CLI_NAMES)
    for n in CLI_NAMES:
        (tmp_path / (n + ".jpg")).write_bytes(LC.jpeg(n))
    extra = ["--pipeline", "--batch", "6"] if mode == "pipeline" else []
    p = subprocess.run([EXE, "--libjpeg"] + extra + [str(tmp_path / (n + ".jpg")) for n in CLI_NAMES], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "Error" not in p.stdout, p.stdout + p.stderr
    for n in CLI_NAMES:
        got = np.frombuffer((tmp_path / (n + ".bmp")).read_bytes(), np.uint8)
        _same(got, want(n)[1], "bmp", (mode, n))


def _pipe(names, datas, **kw):
    import pjd_amd
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            assert index not in got
            got[index] = (name, log, status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=datas, names=[n + ".jpg" for n in names], image_flags=pjd_amd.F_LIBJPEG, sink=sink, **kw)
    assert len(got) == len(names) and all(got[k][0] == n + ".jpg" for k, n in enumerate(names))
    return st, got


def test_batcher_with_image_flags_libjpeg():
    import pjd_amd
    assert len(PIPE_NAMES) == 30 == len(set(PIPE_NAMES))
    _all_with_good_status(PIPE_NAMES)
    st, got = _pipe(PIPE_NAMES, [LC.jpeg(n) for n in PIPE_NAMES], out_format=pjd_amd.OUT_RGB8, batch_images=7, slots=2)
    assert st["n_decoded"] == 30 and st["n_batches"] == 5 and st["n_batch_failures"] == 0 and st["n_rejected"] == 0, st
    for k, n in enumerate(PIPE_NAMES):
        assert got[k][2] == 0, n
        _same(got[k][3].reshape(want(n)[1].shape), want(n)[1], "rgb8", n)


# ---- a picture outside the mode's envelope among good ones ---------------------------------------------------------------------------------
MIXED = ["e259x37_420", "s19x7_420", "sat67x35_444_q30", "h1v2_48x64", "e257x19_grey", "e11x2_422", "e200x150_444_ri25"]
REASON = "Error - PJD_F_LIBJPEG does not take 4:4:0 (h1v2) sampling"


def _mixed_bytes(n):
    return golden_bytes(n) if n.startswith("h1v2") else LC.jpeg(n)


@pytest.mark.parametrize("mode", ["plain", "pipeline"])
def test_cli_leaves_out_the_one_picture_the_flag_does_not_take(tmp_path, mode):
    """h1v2_48x64 (4:4:0) in the middle of six good files: it is reported with the planner's reason and gets no BMP; the six decode."""
    for n in MIXED:
        (tmp_path / (n + ".jpg")).write_bytes(_mixed_bytes(n))
    extra = ["--pipeline"] if mode == "pipeline" else []
    p = subprocess.run([EXE, "--libjpeg"] + extra + [str(tmp_path / (n + ".jpg")) for n in MIXED], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    refused = str(tmp_path / "h1v2_48x64.jpg")
    assert f"{refused}: {REASON}\n" in p.stdout, p.stdout
    assert p.stdout.count("Error") == 1 and "batch" not in p.stdout.split("Profiles:")[0], p.stdout
    assert not (tmp_path / "h1v2_48x64.bmp").exists()
    n_good = 0
    for n in MIXED:
        if n.startswith("h1v2"):
            continue
        assert want(n)[0] == 0
        _same(np.frombuffer((tmp_path / (n + ".bmp")).read_bytes(), np.uint8), want(n)[1], "bmp", (mode, n))
        n_good += 1
    assert n_good == 6


def test_batcher_leaves_out_the_one_picture_the_flag_does_not_take():
    import pjd_amd
    st, got = _pipe(MIXED, [_mixed_bytes(n) for n in MIXED], out_format=pjd_amd.OUT_BMP, batch_images=7, slots=2)
    assert st["n_batch_failures"] == 0 and st["n_decoded"] == 6 and st["n_rejected"] == 1 and st["n_batches"] == 1, st
    for k, n in enumerate(MIXED):
        name, log, status, data = got[k]
        if n.startswith("h1v2"):
            assert status == -2 and data is None and log.endswith(f"{n}.jpg: {REASON}\n"), (status, log)
        else:
            assert status == 0 and want(n)[0] == 0, n
            _same(data, want(n)[1], "bmp", n)
