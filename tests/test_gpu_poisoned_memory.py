"""Every decode path on poisoned and on stale device memory (run with -m gpu on an MI355X).

The library clears two of the roughly twenty device buffers of a batch; everything else reaches the kernels as hipMalloc or the
context's buffer pool hands it out, and the decode is right only while no kernel reads a word that this decode has not written
(DESIGN.md 5b lists every buffer, its writer, its readers and the guard).  Fresh memory is usually zero and what the pool recycles
depends on test order, so the other suites cannot see a violation.  Here every case opens its own Context under
PJD_DEBUG_POISON=<byte> -- every allocation made for that context is filled with the byte before anything else touches it -- once
with 0xFF (huge counts, negative int16, NaN patterns) and once with 0xA5 (asymmetric: a swapped or half-written field shows), and
compares bit for bit with what the other suites compare with: the oracle port, the recorded reference hashes, the stream writers'
intent and the numpy models of the resize, antialias, window and normalize arithmetic.  The last test runs WITHOUT the switch: a
pooled batch that follows a batch of the same shape, where every stale word is a valid entry of the wrong picture.

The figures of the module (wall time, what the cases catch) are in profiles/poisoned_memory.md."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import jpeg_symbols as J
import normalize_model as nm
import resize_aa_model as aa
import resize_model
import resize_window_model as wm
import stream_cases
import symbol_corpus as SC
from conftest import golden_bytes, ROOT
from test_gpu_scaled import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
HUFF_ERR = sorted(k for k in VALID if MANIFEST[k]["huff_ok"] == 0)
ROUTED = [n for n in VALID if n.startswith("div_rst") or n.startswith("huff_")]       # exact kernel up front (test_gpu_parity: routing)
POISON = [0xFF, 0xA5]
SCALES = [(0, 1), (16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)
DTYPES = [0, nm.DT_F16, nm.DT_BF16, nm.DT_F32]
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    return synth


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def _witness(ctx, byte):
    """The switch is on for this context.  The resized pictures of a batch lie 256-byte aligned in a result buffer that nothing
    clears and that the resample launch writes picture by picture: the packed download brings the gaps between them along, and they
    hold the byte and nothing else."""
    import pjd_amd
    sc = [pjd_amd.Scanned(golden_bytes("gray_61x45")) for _ in range(2)]
    with ctx.batch([s.desc for s in sc]) as b:
        b.set_resize([(5, 7), (5, 7)])
        b.upload(); b.decode()
        size, off, n = b.packed_size(), b.output_offset(1), b.output_size(0)
        host = np.zeros(size, np.uint8)
        st = (C.c_int32 * 2)()
        ctx._check(b.L.pjd_batch_download_packed(b._h, C.c_void_p(host.ctypes.data), size, st), "pjd_batch_download_packed")
    want = resize_model.resize(_fixture("gray_61x45")[1], 7, 5).reshape(-1)
    assert (n, off, size) == (105, 256, 512) and list(st) == [0, 0]
    assert np.array_equal(host[:n], want) and np.array_equal(host[off:off + n], want)
    gaps = np.concatenate([host[n:off], host[off + n:]])
    assert (gaps == byte).all(), (hex(byte), np.unique(gaps)[:8].tolist())


@pytest.fixture(params=POISON, ids=["ff", "a5"])
def poison(request, monkeypatch):
    """The poison byte of this run, with the switch set for every Context opened from here on (in this process and, through the
    environment, in the child processes and in the contexts the pipeline and pjd_split_decode open themselves)."""
    monkeypatch.setenv("PJD_DEBUG_POISON", hex(request.param))
    return request.param


def _open(poison, **kw):
    import pjd_amd
    c = pjd_amd.Context(0, **kw)
    try:
        _witness(c, poison)
    except BaseException:
        c.close()
        raise
    return c


@pytest.fixture
def pctx(poison):
    c = _open(poison)
    yield c
    c.close()


def test_the_switch_takes_decimal_and_hex_and_is_per_context(monkeypatch):
    """PJD_DEBUG_POISON is read in pjd_open: `165` and `0xa5` are the same byte, and a context opened after the variable is gone
    is not poisoned while the one opened before still is."""
    import pjd_amd
    for text in ("165", "0xa5", "0XA5"):
        monkeypatch.setenv("PJD_DEBUG_POISON", text)
        c = pjd_amd.Context(0)
        try:
            _witness(c, 0xA5)
        finally:
            c.close()
    monkeypatch.setenv("PJD_DEBUG_POISON", "0x5c")
    on = pjd_amd.Context(0)
    monkeypatch.delenv("PJD_DEBUG_POISON")
    off = pjd_amd.Context(0)
    try:
        _witness(on, 0x5C)
        sc = [_scanned(golden_bytes(n)) for n in VALID]
        for c in (on, off):
            outs, st = c.decode([s.desc for s in sc], pjd_amd.OUT_BMP)
            _check_fixtures(VALID, outs, st, "bmp")
    finally:
        on.close()
        off.close()


# ---- expectations, computed once per process and never changed ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _port():
    import oracle_lib
    return oracle_lib.Port()


@functools.lru_cache(maxsize=None)
def _oracle(data):
    """The oracle port's answer for one stream: (status, H x W x 3 picture, BMP file bytes, coefficient buffer)."""
    o = _port().decode(data)
    rgb, coef = o["rgb"], o["coef"]
    rgb.setflags(write=False)
    coef.setflags(write=False)
    return o["huff_rc"], rgb, np.frombuffer(bytes(o["bmp"]), np.uint8), coef


def _fixture(name):
    return _oracle(golden_bytes(name))


def _scanned(data, flags=0, options=0):
    import pjd_amd
    s = pjd_amd.Scanned(data, options=options)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _fmt(fmt):
    import pjd_amd
    return {"rgb8": pjd_amd.OUT_RGB8, "bmp": pjd_amd.OUT_BMP, "planar": pjd_amd.OUT_RGB8_PLANAR}[fmt]


def _same(got, want_rgb, fmt, label, want_bmp=None):
    """got, as download() returns it in `fmt`, is the H x W x 3 picture; a BMP file also byte for byte, its row padding zero."""
    if fmt == "bmp":
        import pjd_amd
        want = np.frombuffer(pjd_amd.rgb_to_bmp(want_rgb), np.uint8) if want_bmp is None else want_bmp
        got = np.asarray(got).reshape(-1)
        h, w, _ = want_rgb.shape
        stride = 3 * w + w % 4
        assert got.size == want.size == 26 + h * stride, label
        if w % 4:
            pad = got[26:].reshape(h, stride)[:, 3 * w:]
            assert not pad.any(), (label, "BMP row padding is not zero", np.unique(pad).tolist())
    else:
        want = np.ascontiguousarray(want_rgb.transpose(2, 0, 1)) if fmt == "planar" else want_rgb
        assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (label, fmt, "first differing byte", int(bad[0]), "of", want.size, "differing", int(bad.size),
                           "values there", np.asarray(got).reshape(-1)[bad[:4]].tolist())


def _check_fixtures(names, outs, st, fmt, scale=None):
    assert len(outs) == len(st) == len(names)
    for k, n in enumerate(names):
        status, rgb, bmp, _ = _fixture(n)
        s = scale[k] if scale else 1
        assert st[k] == status, (n, st[k], status)
        _same(outs[k], box(rgb, s), fmt, (n, s), bmp if s == 1 else None)
    return len(names)


def _check_streams(jpegs, outs, st, fmt="rgb8"):
    assert len(outs) == len(st) == len(jpegs)
    n_err = 0
    for k, j in enumerate(jpegs):
        status, rgb, bmp, _ = _oracle(j)
        assert st[k] == status, (k, st[k], status)
        _same(outs[k], rgb, fmt, k, bmp)
        n_err += status != 0
    return n_err


# ---- 1: every fixture in one batch, decoded, decoded again, captured and replayed -------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bmp", "planar"])
@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_fixtures_in_one_batch_decoded_twice_and_replayed(poison, mode, fmt):
    """All decodable fixtures (every sampling, restart intervals, the routed div_rst_* and huff_* ones, the entropy-error ones) in ONE
    batch: pictures and statuses after the first decode, after a second one, and after each of two replays of the captured graph; the
    single chain of launches (the timed decode) gives the same.  107 pictures: on an idle device the plain decodes take the
    picture-group form."""
    import pjd_amd
    c = _open(poison, plan_mode=pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
    try:
        sc = [_scanned(golden_bytes(n)) for n in VALID]
        with c.batch([s.desc for s in sc], _fmt(fmt)) as b:
            b.upload()
            n = 0
            for step in ("decode", "again", "timed", "replay 1", "replay 2"):
                if step == "replay 1":
                    b.capture()
                if step == "timed":
                    b.decode_timed()
                else:
                    b.decode()
                outs, st = b.download()
                n += _check_fixtures(VALID, outs, st, fmt)
            info = b.info()
        assert n == 5 * len(VALID)
        assert info["n_sequential"] == len(ROUTED) == 4 and info["n_fallback"] == 0, info
        assert info["plan_mode"] == (1 if mode == "throughput" else 0)
    finally:
        c.close()


# ---- 2: error paths -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _truncated():
    """Seeded pictures of several lanes and MCU rows cut at a quarter, a half and all but a few bytes of their entropy-coded data."""
    synth = _synth()
    out = []
    for k, sub in enumerate([synth.SUB_420, synth.SUB_444, synth.SUB_GREY]):
        good = synth.make(136, 104, 610 + k, 92, sub, 0, synth.DENSE_DETAIL, bool(k & 1))
        body = good.rfind(b"\xff\xda") + 14
        n = len(good) - 2 - body
        for cut in (n // 4, n // 2, n - 9):
            out.append(good[:body + cut] + b"\xff\xd9")
    return tuple(out)


def test_entropy_error_fixtures_corrupted_and_truncated_streams(pctx):
    """The entropy-error fixtures, the first 64 seeded in-place corrupted streams of test_random_corrupted_streams and truncated
    pictures, in one batch as RGB8 and as BMP: the reference's status and its PARTIAL picture -- the units behind the first error are
    the reference's zeros, which nothing but the upload's clear of the result buffer provides."""
    import pjd_amd
    port = _port()
    jpegs = [golden_bytes(n) for n in HUFF_ERR] + [j for j in stream_cases.corrupted_streams(64) if port.parse(j)["info"]["valid"]] + list(_truncated())
    assert len(jpegs) > 60
    sc = [_scanned(j) for j in jpegs]
    for fmt in ("rgb8", "bmp"):
        with pctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
        assert _check_streams(jpegs, outs, st, fmt) >= len(HUFF_ERR) + len(_truncated()) + 3
        assert info["n_entropy_errors"] > 0


def test_errors_at_lane_edges_and_in_units_that_run_on_into_the_next_lane(poison, monkeypatch):
    """128-byte lanes, as the two tests these streams come from force them: every error class planted within a byte of a lane or a
    checkpoint boundary (test_errors_at_lane_and_checkpoint_edges: status, picture and coefficients against the intent), and every
    eighth stream of test_error_in_a_unit_that_runs_on_into_the_next_lane (the lane behind the error holds entries the reference
    never decoded)."""
    import pjd_amd
    from test_gpu_symbol_streams import _decode_and_check, _edge_streams, _scan
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    items = _edge_streams()
    assert len(items) >= 40 and {it.status for *_, it in items} == set(range(1, 8))
    jpegs = list(stream_cases.runon_error_streams()[::8])
    assert len(jpegs) >= 30
    c = _open(poison)
    try:
        info = _decode_and_check(c, _port(), items, _scan(items))
        assert info["sub_bytes"] == 128
        sc = [_scanned(j) for j in jpegs]
        with c.batch([s.desc for s in sc]) as b:
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
            n_ac = sum(s in (4, 6) for s in st)                 # PJD_ST_AC_SYM / PJD_ST_AC_LEN: the unit stays open at the error
            assert _check_streams(jpegs, outs, st) >= n_ac > len(jpegs) // 2
            for k in range(0, len(jpegs), 5):
                assert np.array_equal(b.coefficients(k), _oracle(jpegs[k])[3]), k
        assert info["sub_bytes"] == 128 and info["n_sequential"] == 0 and info["n_fallback"] == 0, info
    finally:
        c.close()


# ---- 3: pictures the parallel decoder flags, routed pictures, the exact kernel for everything -----------------------------------------------
@functools.lru_cache(maxsize=1)
def _misplaced_restart_markers():
    """Restart-segmented fixtures with one byte inserted before, or the byte removed before, a restart marker in the middle of the
    stream: a segment that ends late or early without an entropy-coding error of its own, which the parallel decoder does not settle
    (PJD_FLAG_SEGMENT) -- the exact kernel decodes the picture again into the scratch settle() allocates."""
    out = []
    for name in ("rst4_128x96_444", "rstrow_200x150_444_opt", "rstrow_gray_100x60"):
        good = golden_bytes(name)
        body = good.rfind(b"\xff\xda") + 14
        marks = [i for i in range(body, len(good) - 2) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
        assert len(marks) >= 3, name
        for m in (marks[len(marks) // 2], marks[1]):
            out.append(good[:m] + b"\x00" + good[m:])
            if good[m - 1] not in (0x00, 0xFF) and good[m - 2] != 0xFF:
                out.append(good[:m - 1] + good[m:])
    return tuple(j for j in out if _port().parse(j)["info"]["valid"])


def test_flagged_and_routed_pictures(pctx):
    """(a) Streams whose restart markers are a byte off: at least one picture is flagged by the parallel decoder and decoded again
    by the exact kernel (n_fallback), with the oracle's status, picture and coefficients -- also on a second decode of the batch.
    (b) The first 60 error streams of the symbol corpus, which the parallel decoder settles without a re-decode.  (c) The routed
    pictures of test_subsampled_restart_under_the_reference_rule_is_routed."""
    import pjd_amd
    from test_gpu_int16_edges import family
    from test_gpu_symbol_streams import _decode_and_check, _scan
    jpegs = list(_misplaced_restart_markers())
    assert len(jpegs) >= 6
    sc = [_scanned(j) for j in jpegs]
    assert all(pjd_amd.plan_info([s.desc])["n_sequential"] == 0 for s in sc), "the planner takes them: only the decoder can flag them"
    with pctx.batch([s.desc for s in sc]) as b:
        b.upload()
        for rep in range(2):
            b.decode()
            outs, st = b.download()
            info = b.info()
            _check_streams(jpegs, outs, st)
            assert info["n_fallback"] >= 1 and info["n_sequential"] == 0 and sum(info["flag_waves"]) >= info["n_fallback"], (rep, info)
        for k, j in enumerate(jpegs):
            assert np.array_equal(b.coefficients(k), _oracle(j)[3]), k
    items = [x for x in SC.corpus() if x[3].status != J.OK][:60]
    info = _decode_and_check(pctx, _port(), items, _scan(items))
    assert info["n_entropy_errors"] > 0, info
    routed = [x for x in family() if x[2].ri and not x[2].standard_restart and (x[2].hs, x[2].vs) != (1, 1)]
    assert len(routed) >= 2
    info = _decode_and_check(pctx, _port(), routed, _scan(routed))
    assert info["n_sequential"] == len(routed)


@pytest.mark.parametrize("fmt", ["rgb8", "bmp"])
def test_every_fixture_under_force_sequential(poison, monkeypatch, fmt):
    """PJD_FORCE_SEQUENTIAL=1: every picture goes to the exact kernel and the dense back end, no descriptor says so."""
    import pjd_amd
    monkeypatch.setenv("PJD_FORCE_SEQUENTIAL", "1")
    c = _open(poison)
    try:
        sc = [_scanned(golden_bytes(n)) for n in VALID]
        with c.batch([s.desc for s in sc], _fmt(fmt)) as b:
            b.upload()
            for rep in range(2):
                b.decode()
                outs, st = b.download()
                _check_fixtures(VALID, outs, st, fmt)
            info = b.info()
            bad = [n for i, n in enumerate(VALID) if hashlib.sha256(b.coefficients(i).tobytes()).hexdigest() != MANIFEST[n]["coef_sha256"]]
        assert info["n_sequential"] == len(VALID) and info["n_huff_waves"] == 0, info
        assert not bad, bad
    finally:
        c.close()


# ---- 4: the other forms of the back end -----------------------------------------------------------------------------------------------------
def test_picture_groups_with_damaged_pictures(pctx):
    """128 pictures (the lane-path fixtures and the first corrupted streams): on an idle device the decode takes the picture-group
    form, a group's DC scan and back end read lane_info, marks and error state of its own pictures only."""
    import pjd_amd
    port = _port()
    jpegs = [golden_bytes(n) for n in VALID if n not in ROUTED]
    jpegs += [j for j in stream_cases.corrupted_streams(40) if port.parse(j)["info"]["valid"]]
    jpegs = jpegs[:128]
    assert len(jpegs) == 128
    sc = [_scanned(j) for j in jpegs]
    assert pjd_amd.plan_info([s.desc for s in sc])["n_sequential"] <= 128 - 64      # damaged streams under the reference's restart rule are routed
    with pctx.batch([s.desc for s in sc], pjd_amd.OUT_BMP) as b:
        b.upload()
        for step in ("decode", "replay"):
            if step == "replay":
                b.capture()
            b.decode()
            outs, st = b.download()
            assert b.info()["dc_plan"] >> 8 == 3 and b.decode_chains() == 3, (step, b.info()["dc_plan"] >> 8, b.decode_chains())
            assert _check_streams(jpegs, outs, st, "bmp") >= 10, step


CHILD = """
import os, sys
sys.path[:0] = %(path)r
import numpy as np, pjd_amd
import test_gpu_poisoned_memory as T
c = T._open(%(poison)d)
jpegs = [T.golden_bytes(n) for n in T.VALID if n not in T.ROUTED]
jpegs += [j for j in T.stream_cases.corrupted_streams(24) if T._port().parse(j)["info"]["valid"]]
sc = [T._scanned(j) for j in jpegs]
b = c.batch([s.desc for s in sc], pjd_amd.OUT_RGB8)
b.upload()
n_err = 0
for step in ("decode", "replay 1", "replay 2"):
    if step == "replay 1":
        b.capture()
    b.decode(); b.sync()
    outs, st = b.download()
    n_err += T._check_streams(jpegs, outs, st)
assert np.array_equal(b.coefficients(0), T._oracle(jpegs[0])[3])
info = b.info()
b.destroy(); c.close()
print("RESULT ok", len(jpegs), n_err, info["n_fallback"], info["walks"])
"""


def _child(poison, env):
    e = dict(os.environ, PJD_DEBUG_POISON=hex(poison), **env)
    code = CHILD % {"path": [os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"), HERE, os.path.join(ROOT, "tools")], "poison": poison}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-600:] + r.stderr[-3000:])
    return [int(v) for v in r.stdout.split("RESULT ok")[1].split()]


@pytest.mark.parametrize("walk_max", ["64", "0"])
def test_walker_forced_on_and_off(poison, walk_max):
    """PJD_WALK_MAX=64: every re-sync round of every picture is a cooperative walk; 0: never.  The same batch, the same checks."""
    n, n_err, _, walks = _child(poison, {"PJD_WALK_MAX": walk_max})
    assert n >= 100 and n_err >= 3 * (len(HUFF_ERR) - 2)
    assert (walks > 0) == (walk_max == "64"), walks


def test_128_byte_lanes(poison, monkeypatch):
    """PJD_SUB_BYTES=128: the shortest lanes, the most lane_info and mark words per picture; fixtures and damaged streams."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    c = _open(poison)
    try:
        sc = [_scanned(golden_bytes(n)) for n in VALID]
        with c.batch([s.desc for s in sc], pjd_amd.OUT_BMP) as b:
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
        _check_fixtures(VALID, outs, st, "bmp")
        assert info["sub_bytes"] == 128 and info["n_sequential"] == len(ROUTED), info
    finally:
        c.close()


# ---- 5: reduced size ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bmp", "planar"])
def test_reduced_sizes_mixed_in_one_batch(pctx, fmt):
    """Every fixture, the scales 1, 1/2, 1/4 and 1/8 round-robin in one batch: the box filter of the oracle's picture."""
    sc = [_scanned(golden_bytes(n), SCALES[k % 4][0]) for k, n in enumerate(VALID)]
    with pctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload(); b.decode()
        outs, st = b.download()
    assert _check_fixtures(VALID, outs, st, fmt, [SCALES[k % 4][1] for k in range(len(VALID))]) == len(VALID)


# ---- 6: progressive frames ------------------------------------------------------------------------------------------------------------------
def test_progressive_valid_and_broken_streams(pctx):
    """The small valid streams and every ninth broken one of tests/progressive_corpus.py: the coefficient buffer accumulates over the
    scans of a frame, so status, coefficients and picture depend on its clear -- decoded twice."""
    import test_gpu_progressive_streams as TP
    items = TP.valid_items() + TP.broken_items()[::9]
    assert len(items) > 140
    scanned = TP.scan_all(items)
    with pctx.batch([s.desc for s in scanned]) as b:
        b.upload()
        for rep in range(2):
            b.decode(); b.sync()
            outs, st = b.download()
            assert TP.check_batch(_port(), b, items, outs, st) == len(items), rep
        assert b.info()["n_sequential"] == len(items)


# ---- 7, 8: coefficients, the DPU payload ----------------------------------------------------------------------------------------------------
def test_coefficients_of_lane_path_and_exact_path_pictures(pctx):
    """pjd_batch_download_coefficients allocates its result (and, for a re-decoded picture, a scratch) outside the pool: a lane-path
    pictures, two routed ones, an entropy-error one and a grey one against the reference's recorded hashes and the oracle."""
    import pjd_amd
    names = ["big_640x480_420_q85", "rstrow_200x150_444_opt", "div_rst_420_64x48", "huff_oversub_96x64_444", "err_corrupt_3", "gray_33x70"]
    sc = [_scanned(golden_bytes(n)) for n in names]
    with pctx.batch([s.desc for s in sc]) as b:
        b.upload(); b.decode(); b.sync()
        info = b.info()
        for i, n in enumerate(names):
            got = b.coefficients(i)
            assert hashlib.sha256(got.tobytes()).hexdigest() == MANIFEST[n]["coef_sha256"], n
            assert np.array_equal(got, _fixture(n)[3]), n
    assert info["n_sequential"] == 2 and info["n_fallback"] == 0


def test_dpu_payload_on_the_smallest_fixture(pctx):
    name = min(VALID, key=lambda n: (MANIFEST[n]["dims"][0] * MANIFEST[n]["dims"][1], n))
    o = _port().decode(golden_bytes(name))
    n = o["coef"].shape[0]
    mcus = o["coef"].copy()
    pctx.exec_dpu_payload(np.tile(o["metadata"], (n, 1)), mcus)
    assert n >= 1 and np.array_equal(mcus, o["mcus"]), name


# ---- 9: split decode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bmp"])
def test_split_decode_over_duplicated_ordinals(poison, monkeypatch, fmt):
    """pjd_split_decode opens a context per rank itself (they read the switch) and allocates the descriptor blob of every rank: a
    restart-segmented picture over 2, 3 and 5 ranks on one device, a range boundary inside an MCU row among them."""
    import pjd_amd
    monkeypatch.setenv("PJD_PIPE_ALLOW_DUP_DEVICES", "1")
    try:
        for name in ("rst4_128x96_444", "rstrow_gray_100x60"):
            status, rgb, bmp, _ = _fixture(name)
            s = _scanned(golden_bytes(name))
            for world in (2, 3, 5):
                got, st, stats = pjd_amd.split_decode(s.desc, [0] * world, _fmt(fmt))
                assert st == status == 0 and stats["redone_whole"] == 0 and stats["n_exact"] == 0, (name, world, stats)
                assert stats["n_ranks"] == min(world, int(s.desc.n_segments)), (name, world, stats)
                _same(got, rgb, fmt, (name, world), bmp)
    finally:
        pjd_amd.dev_lib().pjd_split_release()


# ---- 10: the pipelined batcher --------------------------------------------------------------------------------------------------------------
def test_pipeline_over_the_fixtures_in_memory(poison):
    """pjd_pipe_release() first, so that the slots' contexts are opened under the switch (and again afterwards, so that they do not
    outlive it): every fixture through two slots in batches of seven, the reference's BMP hashes."""
    import pjd_amd
    names = sorted(MANIFEST)
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            got[index] = (status, None if data is None else hashlib.sha256(data.tobytes()).hexdigest())

    pjd_amd.pipe_lib()
    pjd_amd.pipe_release()
    try:
        st = pjd_amd.pipe_run(jpegs=[golden_bytes(n) for n in names], names=[n + ".jpg" for n in names], out_format=pjd_amd.OUT_BMP,
                              batch_images=7, scan_threads=3, slots=2, sink_threads=3, sink=sink)
    finally:
        pjd_amd.pipe_release()
    assert st["n_decoded"] == len(VALID) and st["n_rejected"] == len(names) - len(VALID) and st["n_batch_failures"] == 0, st
    assert st["n_exact_images"] == len(ROUTED), st
    for i, n in enumerate(names):
        ent = MANIFEST[n]
        if ent["rc"] != 0:
            assert got[i] == (-1, None), n
        else:
            assert got[i][1] == ent["bmp_sha256"] and (got[i][0] == 0) == bool(ent["huff_ok"]), n


# ---- 11: resize on decode, unbound ----------------------------------------------------------------------------------------------------------
def W(x=0, y=0, w=0, h=0, vw=0, vh=0, ox=0, oy=0, flip=False):
    return {k: v for k, v in dict(x=x, y=y, w=w, h=h, vw=vw, vh=vh, ox=ox, oy=oy, flags=wm.HFLIP if flip else 0).items() if v}


ERR_PICTURE = "err_truncated_eoi_420"          # in every resize batch: the resample reads a partly written intermediate


@functools.lru_cache(maxsize=None)
def _resize_cases(kind):
    """[(jpeg bytes, window or None, (th, tw), status, th x tw x 3 uint8 expectation)]: the tile-edge geometry the resize suites name.
    bilinear: test_resize_targets_around_the_tile_edges; antialias: GEOMETRY of test_gpu_resize_aa; window: the mirrored and offset
    cases of GEOMETRY of test_gpu_resize_window, with the antialiased filter on (its windowed kernels stage rows in LDS)."""
    synth = _synth()
    cases = []
    if kind == "bilinear":
        data = golden_bytes("big_640x480_420_q85")
        cases = [(data, None, (th, tw)) for tw, th in [(255, 7), (256, 8), (257, 9), (511, 15), (513, 17), (256, 17), (257, 7)]]
        cases.append((golden_bytes(ERR_PICTURE), None, (33, 21)))
    elif kind == "antialias":
        from test_gpu_resize_aa import GEOMETRY
        cases = [(synth.make(w, h, seed, 90, synth.SUB_444), None, (th, tw)) for (w, h, seed), (tw, th) in GEOMETRY]
        cases.append((golden_bytes(ERR_PICTURE), None, (9, 13)))
    else:
        from test_gpu_resize_window import GEOMETRY
        pick = [g for g in GEOMETRY if g[1].get("flags") or g[1].get("ox")]
        assert len(pick) >= 6
        for pic, win, (tw, th) in pick:
            data = golden_bytes(pic) if isinstance(pic, str) else synth.make(pic[0], pic[1], pic[2], 90, synth.SUB_444)
            cases.append((data, win, (th, tw)))
        cases.append((golden_bytes(ERR_PICTURE), W(3, 2, 40, 30, flip=True), (11, 17)))
    out = []
    for data, win, (th, tw) in cases:
        status, rgb, _, _ = _oracle(data)
        if kind == "bilinear":
            want = resize_model.resize(rgb, tw, th)
        elif kind == "antialias":
            want = aa.resize(rgb, tw, th)
        else:
            want = wm.window(rgb, win, tw, th, True)
        want.setflags(write=False)
        out.append((data, win, (th, tw), status, want))
    assert out[-1][3] != 0
    return tuple(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
@pytest.mark.parametrize("kind", ["bilinear", "antialias", "window"])
def test_resize_on_decode_into_the_batch_s_own_buffers(pctx, kind, fmt, dtype):
    """Bilinear, antialiased, and windowed with a flip, as uint8 and as fp16 / bf16 / fp32, interleaved and planar, into the batch's
    own result buffer: the work list, the weight table, the window records, the intermediate and the result all come from the pool.
    Every element of every target equals the model (for floats: the normalize model over it, bit for bit) -- none is the poison."""
    import pjd_amd
    from pjd_amd import tensors
    planar = fmt == "planar"
    cases = _resize_cases(kind)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    sc = [_scanned(data) for data, _, _, _, _ in cases]
    with pctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.set_resize([t for _, _, t, _, _ in cases])
        if kind == "window":
            b.set_resize_window([w for _, w, _, _, _ in cases])
        if kind != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        if dtype:
            b.set_normalize(dtype, scale, bias)
        b.upload()
        for rep in range(2):
            b.decode()
            outs, st = b.download()
            for k, ((_, win, (th, tw), status, u8), o) in enumerate(zip(cases, outs)):
                want = nm.normalize(u8, dtype, scale, bias) if dtype else u8
                want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
                assert st[k] == status, (k, rep)
                assert o.shape == want.shape and o.dtype == want.dtype, (k, o.shape, want.shape, o.dtype)
                bad = np.argwhere(nm.bits(o) != nm.bits(want)) if dtype else np.argwhere(o != want)
                assert bad.size == 0, (kind, fmt, DT_NAME[dtype], k, win, tw, th, rep, "first differing element", bad[0].tolist(), "differing", len(bad))
                if dtype in (nm.DT_F16, nm.DT_F32):
                    assert np.isfinite(o).all(), k


# ---- 12: downloads --------------------------------------------------------------------------------------------------------------------------
def test_download_packed_equals_download(pctx):
    """The packed download copies the whole result buffer, the gaps between the pictures included, into page-locked memory."""
    import pjd_amd
    names = VALID[:9] + HUFF_ERR[:2]
    sc = [_scanned(golden_bytes(n)) for n in names]
    with pctx.batch([s.desc for s in sc], pjd_amd.OUT_BMP) as b:
        b.upload(); b.decode(); b.sync()
        a, sa = b.download()
        p, sp = b.download_packed()
    assert sa == sp
    for n, x, y in zip(names, a, p):
        assert np.array_equal(x, y), n
    _check_fixtures(names, p, sp, "bmp")


# ---- a pooled batch behind a batch of the same shape: stale words that are valid entries of the wrong picture, no switch -------------------
@functools.lru_cache(maxsize=1)
def _twins():
    """(clean, damaged): six seeded pictures of several lanes and MCU rows each, and the same files with one byte of the entropy-coded
    data changed in place -- not to or from 0xFF and not beside one, so byte lengths, headers, stream lengths and with them the plan
    and every allocation size stay -- near the start of the stream (0, 1), in its last lane (2, 3), in the middle (4); picture 5
    stays clean.  The byte and its value are the first from the seeded position on that give the reference an entropy-coding error
    (most changes of one byte fall back into step and only garble a few units)."""
    synth = _synth()
    subs = [synth.SUB_420, synth.SUB_444, synth.SUB_422, synth.SUB_GREY, synth.SUB_440, synth.SUB_444]
    clean, damaged = [], []
    for k, sub in enumerate(subs):
        good = synth.make(168 + 8 * k, 120 + 16 * (k % 3), 900 + k, 93, sub, 5 if k == 5 else 0, synth.DENSE_DETAIL, bool(k & 1))
        body = good.rfind(b"\xff\xda") + 14
        n = len(good) - 2 - body
        bad = good
        if k < 5:
            pos = body + {0: n // 20, 1: n // 9, 2: n - 60, 3: n - 110, 4: n // 2}[k]
            bad = None
            for p in range(pos, pos + 48):
                if 0xFF in good[p - 1:p + 2]:
                    continue
                for v in (good[p] ^ 0x5A, good[p] ^ 0xA5, 0xFE, 0x00):
                    if v not in (0xFF, good[p]) and _port().decode(good[:p] + bytes([v]) + good[p + 1:])["huff_rc"] != 0:
                        bad = good[:p] + bytes([v]) + good[p + 1:]
                        break
                if bad:
                    break
            assert bad, k
        clean.append(good)
        damaged.append(bad)
    return tuple(clean), tuple(damaged)


def _twin_check(b, jpegs, sizes):
    outs, st = b.download()
    for k, j in enumerate(jpegs):
        status, rgb, _, _ = _oracle(j)
        assert st[k] == status, (k, st[k], status)
        want = resize_model.resize(rgb, sizes[k][1], sizes[k][0]) if sizes else rgb
        _same(outs[k], want, "rgb8", k)
    return st


@pytest.mark.parametrize("resize", [False, True], ids=["plain", "resized"])
@pytest.mark.parametrize("first", ["clean", "damaged"])
@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_pooled_twin_sees_plausible_stale_state(mode, first, resize):
    """Batch A is decoded, checked and destroyed; batch B, of the same plan and the same allocation sizes, takes A's blocks from the
    context's pool -- its result buffer is at A's address, which is asserted -- so every lane_info, mark, entry, predictor and status
    word B has not written yet is a perfectly valid word of A's pictures.  B's statuses and pictures must be the oracle's all the
    same.  A clean and B damaged (B's undecoded units lie over A's decoded ones), and the other way round; with a resize on both."""
    import pjd_amd
    clean, damaged = _twins()
    A, B = (clean, damaged) if first == "clean" else (damaged, clean)
    n_bad = sum(_oracle(j)[0] != 0 for j in damaged)
    assert n_bad == 5 and _oracle(damaged[5])[0] == 0 and all(_oracle(j)[0] == 0 for j in clean), [_oracle(j)[0] for j in damaged]
    sizes = [(97 + 3 * k, 131 - 5 * k) for k in range(len(clean))] if resize else None
    c = pjd_amd.Context(0, plan_mode=pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
    try:
        seen = []
        for jpegs in (A, B):
            sc = [_scanned(j) for j in jpegs]
            with c.batch([s.desc for s in sc]) as b:
                if resize:
                    b.set_resize(sizes)
                b.upload(); b.decode()
                st = _twin_check(b, jpegs, sizes)
                info = b.info()
                seen.append((b.device_output(0), info["device_bytes"], info["n_subsequences"], info["n_fallback"], st))
                assert info["n_subsequences"] > 8 * len(jpegs) and info["n_sequential"] == 0, info
        assert seen[1][0] == seen[0][0], "the pool did not hand batch B the result buffer of batch A"
        assert seen[1][1:3] == seen[0][1:3], "the twins do not have the same plan"
    finally:
        c.close()
