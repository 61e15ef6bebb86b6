"""PJD_F_LIBJPEG on progressive frames, and grey output of progressive frames, on the GPU (run with -m gpu on an MI355X).  A
progressive frame always takes the dense front end: a flagged one decodes through pjd_k_idct_std_dense (PJD_OUT_GRAY8:
pjd_k_idct_gray_std_dense) and pjd_k_colour_std, an unflagged grey one through pjd_k_idct_gray.

Every comparison is byte equality, and nothing expected is something this library delivered:

* the fixtures of tests/golden/libjpeg_progressive/ -- complete scan scripts no encoder writes, several back-end ranges, every
  sampling, widths past 256 and 512, the widths where fancy upsampling switches off, saturating content, slot 48 in a scan of its own
  -- against PILLOW'S recorded decode, colour and draft("L");
* the hand-built corpus of tests/progressive_corpus.py, its broken streams and the int16-edge streams of tests/jpeg_progressive.py
  against tests/libjpeg_model.py over the coefficients of the bit-level model (tests/libjpeg_progressive_corpus.py; held to Pillow
  and to pjd_libjpeg_idct by tests/test_libjpeg_progressive_cpu.py) -- incomplete and broken frames are the library's own
  definition, not libjpeg's (include/pjd.h, ENVELOPE);
* unflagged pictures against the oracle port's back end over the same coefficients, as tests/test_gpu_progressive_streams.py and
  tests/gray_expected.py compute it.

No picture is left out of a comparison, and every test asserts how many it compared."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import gray_expected as G
import libjpeg_progressive_corpus as LP
import progressive_corpus as PC
import test_gpu_poisoned_memory as TPM
from conftest import ROOT
from test_gpu_progressive_streams import scan_progressive
from test_gpu_symbol_streams import intent_rgb
from test_libjpeg_cpu import baseline_cases, fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(ROOT, "bin", "decoder")
FORMATS = ["rgb8", "planar", "bmp", "gray8"]
N_FIXTURES, N_CORPUS, N_REFUSED = 18, 46, 9


def _fmt(fmt):
    import pjd_amd
    return pjd_amd.OUT_GRAY8 if fmt == "gray8" else TPM._fmt(fmt)


def same(got, rgb, plane, fmt, label):
    if fmt == "gray8":
        assert got.shape == plane.shape and got.dtype == np.uint8, (label, got.shape, plane.shape)
        bad = np.flatnonzero(got.reshape(-1) != plane.reshape(-1))
        assert bad.size == 0, (label, fmt, "first differing byte", int(bad[0]), "of", plane.size, "differing", int(bad.size))
    else:
        TPM._same(got, rgb, fmt, label)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


# ---- rows: (label, jpeg, flags on top of what the scanner sets, scan options, status, picture, plane) --------------------------------------
_ORACLE = {}


def oracle_expected(port, data, fr):
    """(status, picture, grey plane) of an UNFLAGGED progressive stream: the oracle port's back end over the model's coefficients under
    the T.81 zigzag, as test_gpu_progressive_streams.expected computes it (the baseline twin carries the frame's own quantisers), and
    gray_expected's plane over the same coefficients."""
    if data not in _ORACLE:
        status, coef = LP.model_coefficients(data, fr)
        twin = PC.twin(fr)
        port.standard_zigzag(True)
        try:
            rgb = intent_rgb(port, twin, fr, LP.decoded(data).as_intent())
            plane = G.ref_plane_of_coefficients(port, twin, coef)
        finally:
            port.standard_zigzag(False)
        for a in (coef, rgb, plane):
            a.setflags(write=False)
        _ORACLE[data] = (status, coef, rgb, plane)
    return _ORACLE[data]


def fixture_rows():
    """the committed members, flagged, against Pillow's record"""
    import pjd_amd
    rows = [(n, data, pjd_amd.F_LIBJPEG, True, 0) + LP.record(n) for n, data, _, _ in LP.fixtures()]
    assert len(rows) == N_FIXTURES
    return rows


def baseline_rows():
    """the baseline members of tests/golden/libjpeg/, flagged, against Pillow's record"""
    import pjd_amd
    rows = [(n, fixture(n)[0], pjd_amd.F_LIBJPEG, False, 0, fixture(n)[1], G.l8(n)) for n in baseline_cases() + ["lj_136x72_420_q90_rst4"]]
    assert len(rows) == 16
    return rows


def unflagged_fixture_rows(port):
    rows = [(n + ":plain", data, 0, True) + tuple(oracle_expected(port, data, fr)[k] for k in (0, 2, 3)) for n, data, fr, _ in LP.fixtures()]
    assert len(rows) == N_FIXTURES
    return rows


def model_rows(items):
    """hand-built streams, flagged, against the model"""
    import pjd_amd
    return [(label, data, pjd_amd.F_LIBJPEG, True) + tuple(LP.model_expected(data, fr)[k] for k in (0, 2, 3)) for label, data, fr in items]


def scan_rows(rows, extra=0):
    """The Scanned objects of rows (they own the memory their descriptors point into: keep the list while a batch uses it)."""
    import pjd_amd
    out = []
    for label, data, flags, progressive, *_ in rows:
        if progressive:
            out.append(scan_progressive(data, flags | extra))
        else:
            s = pjd_amd.Scanned(data)
            assert s.valid, label
            s.desc.flags = int(s.desc.flags) | flags | extra
            out.append(s)
    return out


def check(rows, outs, st, fmt, what=""):
    assert len(outs) == len(st) == len(rows)
    for k, (label, _, _, _, status, rgb, plane) in enumerate(rows):
        assert st[k] == status, (label, what, st[k], status)
        same(outs[k], rgb, plane, fmt, (label, what))
    return len(rows)


def check_coefficients(b, items, first=0):
    """status and coefficients of items[k] (picture first + k): what the unflagged decode is held to -- the flag changes no coefficient"""
    for k, (label, data, fr) in enumerate(items):
        _, coef = LP.model_coefficients(data, fr)
        bad = np.argwhere(b.coefficients(first + k) != coef)
        assert bad.size == 0, (label, "coefficients differ from the model at", bad[:4].tolist())
    return len(items)


# ---- 1: the fixtures against Pillow's record -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_fixtures_equal_pillows_record_beside_baseline_and_unflagged_pictures(ctx, port, fmt):
    """One batch: every fixture flagged, the flagged baseline pictures of tests/golden/libjpeg/ (they stay on the lane path) and the
    same progressive streams unflagged (the reference's arithmetic).  The two 136 x 72 members and the 259 x 19 one span three back-end
    ranges (PJD_IDCT_MAX_DU = 96 units): fancy upsampling reads chroma across the boundaries, inside and between MCU rows."""
    import pjd_amd
    rows = fixture_rows() + baseline_rows() + unflagged_fixture_rows(port)
    sc = scan_rows(rows)
    with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
        assert check(rows, outs, st, fmt) == 2 * N_FIXTURES + 16
        assert check_coefficients(b, [x[:3] for x in LP.fixtures()]) == N_FIXTURES
        timed, _ = b.decode_timed()
        b.sync()
        outs, st = b.download()
        assert check(rows, outs, st, fmt, "timed") == len(rows)
    assert list(st) == [0] * len(rows)
    assert info["n_sequential"] == 2 * N_FIXTURES and info["n_fallback"] == 0, info
    if fmt == "gray8":
        assert "idct_gray_std" in timed and "idct_gray" in timed and "colour_std" not in timed, timed
    else:
        assert "idct_std" in timed and "colour_std" in timed, timed
    big = [s for s, r in zip(sc, rows) if r[0].startswith("lp_136x72") and not r[0].endswith(":plain")]
    assert len(big) == 2 and all(pjd_amd.plan_info([s.desc], _fmt(fmt))["n_data_units"] == 270 > 2 * 96 for s in big)


# ---- 2: the hand-built corpus under the flag ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "gray8"])
def test_corpus_under_the_flag(ctx, fmt):
    """Restart intervals that change between scans, table ids 0 to 3, incomplete scripts, overlapping bands, repeated refinements:
    status and coefficients are those of the unflagged decode, the picture the model's (gray8: its luma plane)."""
    items = LP.corpus_items()
    rows = model_rows(items)
    assert len(rows) == N_CORPUS and all(r[4] == 0 for r in rows)
    sc = scan_rows(rows)
    with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
        assert check(rows, outs, st, fmt) == N_CORPUS
        assert check_coefficients(b, items) == N_CORPUS
    assert info["n_sequential"] == N_CORPUS and info["n_fallback"] == 0, info


# ---- 3: broken streams under the flag -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "gray8"])
def test_broken_streams_under_the_flag(ctx, fmt):
    """Cuts and planted symbols in every procedure, in first, middle and last scans: the status class, the coefficients stored up to
    the error -- those of earlier scans stay -- and the model's picture of them; a unit or slot never decoded is 0."""
    items = LP.broken_items()
    rows = model_rows(items)
    assert len(rows) >= 90 and {r[4] for r in rows} == set(range(1, 8)), sorted({r[4] for r in rows})
    late = [label for (label, data, fr) in items if LP.decoded(data).err_scan >= 2]
    assert len(late) >= 30                                       # an error in a late scan: earlier scans' coefficients are in the picture
    sc = scan_rows(rows)
    with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        assert check(rows, outs, st, fmt) == len(items)
        assert check_coefficients(b, items) == len(items)


# ---- 4: int16 extremes ----------------------------------------------------------------------------------------------------------------------
def test_int16_extremes_flagged_and_in_grey(ctx, port):
    """AC first scans at Al = 13 and a DC of +-4096 << 3: -32768 at slot 0, at slot 52 and elsewhere is a VALUE in a progressive frame,
    not the dense scratch's mark.  Flagged, in rgb8 and gray8, against the model (hence pjd_libjpeg_idct); unflagged in gray8 against
    tests/gray_expected.py."""
    import pjd_amd
    items = LP.edge_items()
    assert len(items) == 2
    for _, data, fr in items:
        coef = LP.model_coefficients(data, fr)[1]
        assert (coef == -32768).sum() >= 8
    rows = model_rows(items)
    plain = [(label + ":plain", data, 0, True) + tuple(oracle_expected(port, data, fr)[k] for k in (0, 2, 3)) for label, data, fr in items]
    n = 0
    for fmt, batch in (("rgb8", rows), ("gray8", rows + plain), ("rgb8", plain)):
        sc = scan_rows(batch)
        with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            n += check(batch, outs, st, fmt)
            check_coefficients(b, items)
    assert n == 2 + 4 + 2


# ---- 5: grey output of progressive frames under the reference's arithmetic ---------------------------------------------------------------------
def test_grey_output_of_the_whole_corpus_under_the_reference_arithmetic(ctx, port):
    """All 55 streams, the 4:4:0 ones included, unflagged: channel 0 of the oracle's picture of the model's coefficients with every
    chroma coefficient zeroed."""
    items = LP.corpus_items() + LP.refused_items()
    assert len(items) == N_CORPUS + N_REFUSED == 55
    rows = [(label, data, 0, True) + tuple(oracle_expected(port, data, fr)[k] for k in (0, 2, 3)) for label, data, fr in items]
    sc = scan_rows(rows)
    with ctx.batch([s.desc for s in sc], _fmt("gray8")) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        assert check(rows, outs, st, "gray8") == 55
        assert check_coefficients(b, items) == 55


# ---- 6: state ---------------------------------------------------------------------------------------------------------------------------------
def state_rows():
    return fixture_rows() + model_rows(LP.corpus_items())


@pytest.mark.parametrize("fmt", ["rgb8", "gray8"])
def test_repeated_decodes_replays_and_the_reverse_order(ctx, fmt):
    """The dense scratch accumulates over the scans of a frame and the planes are rewritten by every decode: three decodes of one
    upload, two replays of the captured graph, then the same list in reverse order."""
    rows = state_rows()
    sc = scan_rows(rows)
    n = 0
    with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload()
        for rep in range(3):
            b.decode(); b.sync()
            outs, st = b.download()
            n += check(rows, outs, st, fmt, rep)
        b.capture()
        for rep in range(2):
            b.decode(); b.sync()
            outs, st = b.download()
            n += check(rows, outs, st, fmt, ("replay", rep))
    rev = rows[::-1]
    sc = scan_rows(rev)
    with ctx.batch([s.desc for s in sc], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        n += check(rev, outs, st, fmt, "reverse")
    assert n == 6 * (N_FIXTURES + N_CORPUS)


@pytest.mark.parametrize("fmt", ["rgb8", "gray8"])
def test_poisoned_memory_changes_nothing(monkeypatch, fmt):
    """Contexts whose allocations start as 0xA5 and as 0x00: the same bytes, the expected ones."""
    rows = state_rows()
    results = []
    for byte in (0xA5, 0x00):
        monkeypatch.setenv("PJD_DEBUG_POISON", hex(byte))
        c = TPM._open(byte)
        try:
            sc = scan_rows(rows)
            with c.batch([s.desc for s in sc], _fmt(fmt)) as b:
                b.upload(); b.decode(); b.sync()
                outs, st = b.download()
                assert check(rows, outs, st, fmt, hex(byte)) == N_FIXTURES + N_CORPUS
            results.append([np.asarray(o).copy() for o in outs])
        finally:
            c.close()
    assert len(results) == 2 and all(np.array_equal(a, b) for a, b in zip(*results))


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    import pjd_amd
    good_rows = fixture_rows()[:3]
    good = scan_rows(good_rows)

    def refused(s, fmt):
        with pytest.raises(pjd_amd.PjdError) as e:
            ctx.batch([good[0].desc, s.desc], _fmt(fmt))
        assert "(-3)" in str(e.value) and "image 1" in str(e.value), str(e.value)

    n = 0
    for fmt in ("rgb8", "gray8"):
        for label, data, fr in LP.refused_items()[:3]:
            s = scan_progressive(data, pjd_amd.F_LIBJPEG)       # (a Scanned owns what its descriptor points to: it has to stay alive)
            assert (s.desc.h_samp, s.desc.v_samp) == (1, 2), label
            refused(s, fmt)
            n += 1
        for flag in (pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_8):
            s = scan_progressive(good_rows[1][1], pjd_amd.F_LIBJPEG | flag)
            refused(s, fmt)
            n += 1
        outs, st = ctx.decode([s.desc for s in good], _fmt(fmt))
        assert check(good_rows, outs, st, fmt, "after the refusals") == 3
    assert n == 10


# ---- 8: the batcher and the CLI -----------------------------------------------------------------------------------------------------------------
def test_batcher_with_scan_progressive_and_image_flags_libjpeg():
    """The fixtures and all 55 corpus streams: the 4:4:0 ones reach the sink with status -2 and no data and count as rejected, the
    rest of their batches decodes."""
    import pjd_amd
    rows = fixture_rows() + model_rows(LP.corpus_items())
    refused = LP.refused_items()
    order = rows[:20] + [None] * 4 + rows[20:50] + [None] * 5 + rows[50:]        # the refused ones inside the batches, not at the end
    it = iter(refused)
    jpegs = [next(it)[1] if r is None else r[1] for r in order]
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            assert index not in got
            got[index] = (log, status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=jpegs, out_format=pjd_amd.OUT_RGB8, batch_images=16, slots=2, sink=sink, scan_options=pjd_amd.SCAN_PROGRESSIVE,
                          image_flags=pjd_amd.F_LIBJPEG)
    assert (st["n_decoded"], st["n_rejected"], st["n_batch_failures"]) == (len(rows), N_REFUSED, 0), st
    n = 0
    for k, r in enumerate(order):
        log, status, data = got[k]
        if r is None:
            assert status == -2 and data is None and "PJD_F_LIBJPEG does not take 4:4:0 (h1v2) sampling" in log, (k, status, log)
            continue
        assert status == r[4], r[0]
        same(data.reshape(r[5].shape), r[5], None, "rgb8", r[0])
        n += 1
    assert n == N_FIXTURES + N_CORPUS and len(got) == n + N_REFUSED


def test_cli_progressive_libjpeg(tmp_path):
    import pjd_amd
    names = ["lp_136x72_420_q50_skew_ri3", "lp_259x19_422_q75_two_bands"]
    by_name = {n: data for n, data, _, _ in LP.fixtures()}
    for n in names:
        (tmp_path / (n + ".jpg")).write_bytes(by_name[n])
    p = subprocess.run([EXE, "--progressive", "--libjpeg"] + [str(tmp_path / (n + ".jpg")) for n in names], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "Error" not in p.stdout, p.stdout + p.stderr
    for n in names:
        assert (tmp_path / (n + ".bmp")).read_bytes() == pjd_amd.rgb_to_bmp(LP.record(n)[0]), n


# ---- 9: downstream ------------------------------------------------------------------------------------------------------------------------------
def _torch_case(case, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "libjpeg_torch_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_progressive_members_through_bound_output_and_resize_with_normalisation():
    """tests/libjpeg_torch_cases.py "progressive": lj_33x31_420_q90_prog and two of the fixtures here through decode_to_tensors and
    through one antialiased resize to 32 x 32 with normalisation, against the existing models over Pillow's record."""
    _torch_case("progressive")
