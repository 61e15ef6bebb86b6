"""Decode tables and lane words are made once per upload (run with -m gpu on an MI355X).

pjd_batch_upload builds the Huffman decode tables of every table set and the transposed word rows of every lane behind the copy of the
batch's blob; no decode builds them again, and the captured graphs hold neither kernel.  A decode is then right
only while nothing between two uploads writes either buffer, while a second upload() rebuilds both, and while a batch that takes the
buffers of a destroyed one from the pool gets its own tables and words before its first decode.  Every case compares with the oracle
port (never with another decode of the library); the figures are in profiles/resident_tables.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_model
import resize_window_model as wm
from conftest import golden_bytes, ROOT
from test_gpu_poisoned_memory import _fmt, _misplaced_restart_markers, _oracle, _same, _scanned, _synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F_STANDARD_RESTART, F_FORCE_SEQUENTIAL = 1, 2      # pjd_amd.F_* (checked in _mixed)


def _plan_mode(mode):
    import pjd_amd
    return pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY


def _check(b, items, fmt="rgb8"):
    """items: [(stream, flags, stream whose oracle decode is the expectation)].  Status and picture of every item."""
    outs, st = b.download()
    assert len(outs) == len(st) == len(items)
    for k, (_, _, ref) in enumerate(items):
        status, rgb, bmp, _ = _oracle(ref)
        assert st[k] == status, (k, st[k], status)
        _same(outs[k], rgb, fmt, k, bmp)
    return st


def _scan(items):
    return [_scanned(j, flags) for j, flags, _ in items]


@functools.lru_cache(maxsize=1)
def _mixed():
    """One 4:2:0, one 4:4:4 and one grey fixture; a 4:2:0 picture with a restart interval of two MCUs under F_STANDARD_RESTART (it
    equals the same picture encoded without DRI, as in test_gpu_parity); a corrupted fixture the parallel decoder settles itself; a
    restart-segmented fixture with a byte inserted before a marker, which the parallel decoder flags and the exact kernel decodes
    again (the decode tables' second reader); a table-irregular fixture routed to the exact kernel up front."""
    import pjd_amd
    assert (pjd_amd.F_STANDARD_RESTART, pjd_amd.F_FORCE_SEQUENTIAL) == (F_STANDARD_RESTART, F_FORCE_SEQUENTIAL)
    synth = _synth()
    pic = synth.picture(64, 48, 4711)
    items = [(golden_bytes(n), 0, golden_bytes(n)) for n in ("env_64x48_420_q100", "env_64x48_444_q85", "gray_64x48")]
    items.append((synth.encode(pic, 90, synth.SUB_420, 2), F_STANDARD_RESTART, synth.encode(pic, 90, synth.SUB_420, 0)))
    items.append((golden_bytes("err_corrupt_3"), 0, golden_bytes("err_corrupt_3")))
    bad = _misplaced_restart_markers()[0]
    items.append((bad, 0, bad))
    items.append((golden_bytes("huff_oversub_96x64_444"), 0, golden_bytes("huff_oversub_96x64_444")))
    return tuple(items)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bmp", "rgb8", "planar"])
@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_repeated_decodes_of_one_upload(mode, fmt):
    """Upload once; decode three times, capture, decode three times: statuses and pictures after every decode, the first and the last
    among them.  One picture ends in the exact kernel after the parallel decoder flagged it, one is routed there up front."""
    import pjd_amd
    items = _mixed()
    c = pjd_amd.Context(0, plan_mode=_plan_mode(mode))
    try:
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc], _fmt(fmt)) as b:
            b.upload()
            for step in range(6):
                if step == 3:
                    b.capture()
                b.decode()
                st = _check(b, items, fmt)
                info = b.info()
                assert info["n_sequential"] == 1 and info["n_fallback"] >= 1, (step, info)
        assert st[4] != 0 and st[6] != 0 and st[:4] == [0, 0, 0, 0], st
    finally:
        c.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_exact_path_pictures_only():
    """Every picture carries F_FORCE_SEQUENTIAL: no Huffman wave, no word rows, and the tables the exact kernel reads come from the
    upload alone.  Decoded twice, captured, decoded again, uploaded again, decoded again."""
    import pjd_amd
    items = [(j, flags | F_FORCE_SEQUENTIAL, ref) for j, flags, ref in _mixed()]
    c = pjd_amd.Context(0)
    try:
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc]) as b:
            b.upload()
            for step in ("decode", "again", "replay", "second upload"):
                if step == "replay":
                    b.capture()
                if step == "second upload":
                    b.upload()
                b.decode()
                _check(b, items)
            info = b.info()
        assert info["n_sequential"] == len(items) and info["n_huff_waves"] == 0 and info["n_fallback"] == 0, info
    finally:
        c.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _many_small():
    """72 pictures of 16 x 16, every sampling, four qualities, every other one with tables of its own: the planner makes picture
    groups for such a batch (64 pictures or more, none of many lanes)."""
    synth = _synth()
    subs = [synth.SUB_420, synth.SUB_444, synth.SUB_422, synth.SUB_GREY, synth.SUB_440]
    out = []
    for k in range(72):
        j = synth.make(16, 16, 3100 + k, (30, 60, 85, 97)[k % 4], subs[k % 5], 0, synth.DENSE_DETAIL if k % 3 == 0 else 1.0, bool(k & 1))
        out.append((j, 0, j))
    return tuple(out)


def _groups_run(want_chains=3):
    import pjd_amd
    items = _many_small()
    c = pjd_amd.Context(0)
    try:
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc]) as b:
            b.upload()
            for step in ("decode", "again", "replay 1", "replay 2"):
                if step == "replay 1":
                    b.capture()
                b.decode()
                _check(b, items)
                assert b.decode_chains() == want_chains, (step, b.decode_chains())
            info = b.info()
        assert info["n_sequential"] == 0 and info["n_fallback"] == 0 and info["n_table_sets"] > 8, info
    finally:
        c.close()
    return len(items)


def _child(call, env):
    """`call` of this module in a fresh process (PJD_IDLE_FORM is read once per process; a context reads PJD_DEBUG_POISON when it opens)."""
    path = [os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"), HERE, os.path.join(ROOT, "tools")]
    code = "import sys\nsys.path[:0] = %r\nimport test_gpu_resident_tables as T\nprint('RESULT ok', T.%s)\n" % (path, call)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-600:] + r.stderr[-3000:])
    return r.stdout.split("RESULT ok")[1].split()


def test_idle_device_forms():
    """The picture-group form a decode takes on an idle device (this process: nothing else is in flight), and PJD_IDLE_FORM=chain in a
    fresh child: no group's chain makes its word rows any more, both forms read the upload's."""
    assert _groups_run() >= 64
    assert int(_child("_groups_run(1)", {"PJD_IDLE_FORM": "chain"})[0]) >= 64


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_request_changes_between_decodes():
    """The resample request of a batch is closed by its upload (include/pjd.h: every setter before upload()): set_resize_window on
    the resident batch is refused and changes nothing -- the decode behind it is the plain resize again.  The request does change
    with a new batch over the same pictures, which takes the first one's buffers from the pool: its windowed pictures are right on
    both of its decodes."""
    import pjd_amd
    items = _mixed()[:4]
    sizes = [(37 + 2 * k, 53 - 3 * k) for k in range(len(items))]
    wins = [dict(x=8, y=4, w=40, h=32, flags=wm.HFLIP), None, dict(x=3, y=5, w=50, h=40), dict(x=0, y=0, w=33, h=47, flags=wm.HFLIP)]

    def check(b, windowed):
        outs, st = b.download()
        for k, (_, _, ref) in enumerate(items):
            status, rgb, _, _ = _oracle(ref)
            th, tw = sizes[k]
            want = wm.window(rgb, wins[k], tw, th) if windowed else resize_model.resize(rgb, tw, th)
            assert st[k] == status == 0, k
            _same(outs[k], want, "rgb8", (k, windowed))

    c = pjd_amd.Context(0)
    try:
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc]) as b:
            b.set_resize(sizes)
            b.upload(); b.decode()
            check(b, False)
            with pytest.raises(pjd_amd.PjdError, match="after upload"):
                b.set_resize_window(wins)
            b.decode()
            check(b, False)
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc]) as b:
            b.set_resize(sizes)
            b.set_resize_window(wins)
            b.upload()
            for rep in range(2):
                b.decode()
                check(b, True)
    finally:
        c.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _table_twins():
    """(A, B): six pictures of one size and sampling, each with Huffman tables fitted to it, and the same six in reverse order -- the
    same plan and the same allocation sizes, but behind every table set, every lane's word rows and every picture of A lie another
    picture's in B."""
    synth = _synth()
    a = tuple(synth.make(64, 48, 5200 + k, (35, 55, 70, 85, 93, 98)[k], synth.SUB_444, 0, synth.DENSE_DETAIL if k & 1 else 1.0, True) for k in range(6))
    assert len({j[:j.rfind(b"\xff\xda")] for j in a}) == 6, "the pictures do not have tables of their own"
    return tuple((j, 0, j) for j in a), tuple((j, 0, j) for j in reversed(a))


def _stale_pool_run():
    import pjd_amd
    A, B = _table_twins()
    c = pjd_amd.Context(0)
    try:
        seen = []
        for items in (A, B):
            sc = _scan(items)                  # the descriptors point into these
            with c.batch([s.desc for s in sc]) as b:
                b.upload(); b.decode()
                _check(b, items)
                if items is B:
                    b.upload(); b.decode()
                    _check(b, items)
                info = b.info()
                assert info["n_table_sets"] == 6 and info["n_sequential"] == 0 and info["n_fallback"] == 0, info
                seen.append((b.device_output(0), info["device_bytes"], info["n_subsequences"]))
        assert seen[1] == seen[0], "batch B did not take batch A's buffers from the pool"
    finally:
        c.close()
    return len(B)


def test_pooled_batch_behind_a_batch_with_other_tables():
    """Batch A is uploaded, decoded and destroyed; batch B, of the same shape but with other pictures and other Huffman tables at
    every place, follows from the pool: the tables and word rows it finds there are valid ones of A.  B is right on its first
    decode, and again after a second upload().  Once more under PJD_DEBUG_POISON in a fresh child."""
    assert _stale_pool_run() == 6
    assert int(_child("_stale_pool_run()", {"PJD_DEBUG_POISON": "0xa5"})[0]) == 6


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_timing_names():
    """decode_timed() reports the launches of a decode: neither table build nor lane words is one of them."""
    import pjd_amd
    items = _mixed()
    c = pjd_amd.Context(0)
    try:
        sc = _scan(items)                  # the descriptors point into these
        with c.batch([s.desc for s in sc]) as b:
            b.upload()
            t, total = b.decode_timed()
            _check(b, items)
        names = set(t["kernels_ms"]) if "kernels_ms" in t else set(t)
        assert not names & {"build_tables", "lane_words"}, names
        assert {"huff_lanes", "dc_scan", "idct_colour"} <= names, names
        assert total > 0
    finally:
        c.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_small_lanes(monkeypatch):
    """PJD_SUB_BYTES=128 on the densest fixture (96 x 80 4:4:4 at quality 100, 37 KB: 103 bytes per data unit): five waves of word rows,
    and a back-end range of 96 units spans more than 32 lanes, so its parse takes several windows.  Beside it the mixed pictures."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    dense = golden_bytes("noise_96x80_444_q100")
    c = pjd_amd.Context(0)
    try:
        s = _scanned(dense)
        with c.batch([s.desc]) as b:
            b.upload()
            for step in range(3):
                if step == 2:
                    b.capture()
                b.decode()
                _check(b, [(dense, 0, dense)])
            info = b.info()
        assert info["sub_bytes"] == 128 and info["n_huff_waves"] >= 5 and info["n_fallback"] == 0, info
        assert info["n_subsequences"] * 96 > 32 * info["n_data_units"], info
        items = _mixed() + ((dense, 0, dense),)
        sc = _scan(items)
        with c.batch([x.desc for x in sc]) as b:
            b.upload()
            for step in range(2):
                b.decode()
                _check(b, items)
            assert b.info()["sub_bytes"] == 128
    finally:
        c.close()
