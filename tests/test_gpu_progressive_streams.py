"""Hand-built progressive (SOF2) scans on the GPU (run with -m gpu on an MI355X): the streams of tests/progressive_corpus.py through
pjd_k_progressive, all with PJD_F_STANDARD_ZIGZAG as the other progressive tests decode.

Expected status and coefficients come from the bit-level model of tests/jpeg_progressive.py (which tests/test_progressive_streams.py
pins to the writer's intent and to the reference's own decode_MCU_component); expected pictures from the oracle port's back end run on
the model's coefficients.  A broken stream must leave the model's state at the error: its status class, the coefficients stored up to
there and the picture they give.  No picture is left out of a comparison, and every test asserts how many it compared."""
import functools
import threading
import time

import numpy as np
import pytest

import jpeg_progressive as P
import jpeg_symbols as J
import progressive_corpus as PC
import symbol_corpus as SC
from test_gpu_scaled import box
from test_gpu_symbol_streams import _scan, intent_rgb

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _twin(sub, w, h):
    return PC.twin(PC.frame_of(sub, w, h))


@functools.lru_cache(maxsize=1)
def valid_items():
    """[(label, data, frame)] of every valid stream but the big one."""
    return [(label, w.data, w.frame) for label, w in PC.corpus()]


@functools.lru_cache(maxsize=1)
def broken_items():
    return [(x[0], x[1], x[2]) for x in PC.broken()] + PC.desynchronised()


@functools.lru_cache(maxsize=None)
def _model(data):
    return P.decode(data)


def expected(port, data, fr):
    """-> (status, coefficients in the download's layout, RGB picture) of the model."""
    d = _model(data)
    it = d.as_intent()
    port.standard_zigzag(True)
    try:
        rgb = intent_rgb(port, _twin(fr.sampling(), fr.width, fr.height), fr, it)
    finally:
        port.standard_zigzag(False)
    return d.status, J.intent_buffer(fr, it), rgb


def scan_progressive(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data, options=pjd_amd.SCAN_PROGRESSIVE)
    assert s.valid and int(s.desc.flags) & pjd_amd.F_PROGRESSIVE, s.log
    s.desc.flags = int(s.desc.flags) | pjd_amd.F_STANDARD_ZIGZAG | flags
    return s


def scan_all(items, flags=0):
    """The Scanned objects of items (they own the memory their descriptors point into: keep the list while a batch uses it)."""
    return [scan_progressive(d, flags) for _, d, _ in items]


def check_batch(port, b, items, outs, st, first=0):
    """Status, coefficients and picture of items[k] (picture first + k of the batch) against the model."""
    for k, (label, data, fr) in enumerate(items):
        status, coef, rgb = expected(port, data, fr)
        assert st[first + k] == status, (label, st[first + k], J.STATUS_NAMES[status])
        bad = np.argwhere(b.coefficients(first + k) != coef)
        assert bad.size == 0, (label, "coefficients differ from the model at", bad[:4].tolist())
        assert np.array_equal(outs[first + k], rgb), label
    return len(items)


def test_valid_streams_in_one_batch_beside_baseline_pictures(port):
    """Fixtures and corpus in ONE batch with the baseline sym_* fixtures: every progressive picture equals the model; the baseline
    neighbours still equal their intent and stay on the lane path (n_sequential counts the progressive pictures only)."""
    import pjd_amd
    prog = valid_items()
    base = [(n, d, fr, it) for n, (d, fr, it) in SC.fixtures().items()]
    assert len(prog) == 55 and len(base) >= 30
    scanned = [scan_progressive(d) for _, d, _ in prog] + _scan(base)
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
            assert check_batch(port, b, prog, outs, st) == 55
            for k, (label, data, fr, it) in enumerate(base, len(prog)):
                assert st[k] == it.status, label
                assert np.array_equal(b.coefficients(k), J.intent_buffer(fr, it)), label
                port.standard_zigzag(fr.standard_zigzag)
                try:
                    assert np.array_equal(outs[k], intent_rgb(port, data, fr, it)), label
                finally:
                    port.standard_zigzag(False)
        assert info["n_sequential"] == len(prog) and info["n_fallback"] == 0, info
    finally:
        ctx.close()


def test_broken_streams_leave_the_state_at_the_error(port):
    """Cuts and planted symbols in every procedure, in first, middle and last scans, at the first and the last block and right after a
    restart: status class, PARTIAL coefficients and picture equal the model's state at the error (later scans are not run)."""
    import pjd_amd
    items = broken_items()
    assert len(items) == len(PC.broken()) + 2 > 800
    classes = {_model(d).status for _, d, _ in items}
    assert classes == set(range(1, 8)), classes
    ctx = pjd_amd.Context(0)
    try:
        scanned = scan_all(items)
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            assert check_batch(port, b, items, outs, st) == len(items)
    finally:
        ctx.close()


def test_repeated_decodes_replays_and_the_reverse_order(port):
    """The kernel accumulates into the dense scratch: the same batch decoded three times, captured and replayed three times gives the same
    pictures and coefficients every time (a scratch that is not cleared shows here); then the same list in reverse order."""
    import pjd_amd
    items = valid_items() + broken_items()[::9]
    ctx = pjd_amd.Context(0)
    try:
        scanned = scan_all(items)
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload()
            for rep in range(3):
                b.decode(); b.sync()
                outs, st = b.download()
                assert check_batch(port, b, items, outs, st) == len(items), rep
            b.capture()
            for rep in range(3):
                b.decode(); b.sync()
                outs, st = b.download()
                assert check_batch(port, b, items, outs, st) == len(items), ("replay", rep)
        rev = items[::-1]
        scanned = scan_all(rev)
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            assert check_batch(port, b, rev, outs, st) == len(rev)
    finally:
        ctx.close()


def test_bmp_planar_and_reduced_size_outputs(port):
    """OUT_BMP, OUT_RGB8_PLANAR and PJD_F_SCALE_1_2 on valid and broken streams: the model's picture as a BMP file, as planes, and its
    box filter."""
    import pjd_amd
    items = valid_items() + broken_items()[::17]
    want = [expected(port, d, fr) for _, d, fr in items]
    ctx = pjd_amd.Context(0)
    try:
        scanned = scan_all(items)
        outs, st = ctx.decode([s.desc for s in scanned], pjd_amd.OUT_BMP)
        for k, (label, _, _) in enumerate(items):
            assert st[k] == want[k][0] and bytes(outs[k]) == pjd_amd.rgb_to_bmp(want[k][2]), label
        outs, st = ctx.decode([s.desc for s in scanned], pjd_amd.OUT_RGB8_PLANAR)
        for k, (label, _, _) in enumerate(items):
            assert st[k] == want[k][0] and np.array_equal(outs[k], want[k][2].transpose(2, 0, 1)), label
        scanned = scan_all(items, pjd_amd.F_SCALE_1_2)
        outs, st = ctx.decode([s.desc for s in scanned], pjd_amd.OUT_RGB8)
        for k, (label, _, _) in enumerate(items):
            assert st[k] == want[k][0] and np.array_equal(outs[k], box(want[k][2], 2)), label
    finally:
        ctx.close()


def test_through_the_pipeline(port):
    """pipe_run(..., scan_options=SCAN_PROGRESSIVE) over valid and broken streams and two files the scanner rejects: every stream is
    decoded (a broken one with its status and partial picture), the rejected ones are counted as such."""
    import pjd_amd
    from conftest import golden_bytes
    items = valid_items() + broken_items()[::17]
    rejected = [golden_bytes("neg_cmyk"), golden_bytes("neg_not_jpeg")]
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            got[index] = (status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=[d for _, d, _ in items] + rejected, out_format=pjd_amd.OUT_RGB8, batch_images=16, slots=2, sink=sink,
                          scan_options=pjd_amd.SCAN_PROGRESSIVE, image_flags=pjd_amd.F_STANDARD_ZIGZAG)
    assert (st["n_decoded"], st["n_rejected"], st["n_batch_failures"]) == (len(items), 2, 0), st
    for k, (label, data, fr) in enumerate(items):
        status, _, rgb = expected(port, data, fr)
        assert got[k][0] == status and np.array_equal(got[k][1].reshape(rgb.shape), rgb), label
    assert got[len(items)] == (-1, None) and got[len(items) + 1] == (-1, None)


def test_the_32768_block_picture(port):
    """2048x1024 grey, alone: EOB10..EOB14 with extra bits all zero and all one, and the flush at 32767 followed by another run.  One
    lane decodes seven scans of 32768 blocks; the time is printed (run with -s to see it)."""
    import pjd_amd
    w = PC.big()
    assert {"eobrun_flushed_at_32767", "eob14_extra_zeros", "eob14_extra_ones", "eob14_first", "eob14_refine"} <= w.forms
    ctx = pjd_amd.Context(0)
    try:
        scanned = scan_progressive(w.data)
        with ctx.batch([scanned.desc]) as b:
            b.upload()
            t0 = time.perf_counter()
            b.decode(); b.sync()
            dt = time.perf_counter() - t0
            outs, st = b.download()
            print(f"\n32768-block progressive picture: {dt * 1e3:.1f} ms for {len(w.scans)} scans")
            assert check_batch(port, b, [(w.name, w.data, w.frame)], outs, st) == 1
            assert np.array_equal(b.coefficients(0), J.intent_buffer(w.frame, w.intent))
    finally:
        ctx.close()
