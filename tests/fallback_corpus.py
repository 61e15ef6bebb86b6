"""Streams that are known to end in the exact-kernel fallback of pjd_batch_sync (settle() in csrc/pjd_api.hip), for
tests/test_fallback_cpu.py and tests/test_gpu_fallback.py.  Everything is generated, nothing committed.  All of them are meant for
128-byte lanes (PJD_SUB_BYTES=128) and are taken by the planner (n_sequential == 0): only the device can flag them.

    falling()      {name: nosync_corpus.Stream}: four streams of tests/nosync_corpus.py whose routes tests/test_gpu_nosync.py records
                   (lock_grey_910, lock_420_130, chain_x5, phase_420_big) and three new class-1 streams in 4:2:2, 4:4:4 and 4:4:0,
                   nine waves of 128-byte lanes each (grey falls back from seven waves on and 4:2:0 from six, DESIGN.md 4.2: nine is
                   margin, not a threshold)
    broken()       the restart-segmented fixtures with a byte inserted or removed in front of a restart marker
                   (test_gpu_poisoned_memory._misplaced_restart_markers: file-level edits, expected through the oracle port)
    shards()       [Shard]: for the two fixtures with one restart segment per MCU row, segment ranges [r0, r1) of a broken stream and
                   the FILE that is that shard -- the segments under a frame header of the shard's height.  DC predictors reset at
                   every restart and the oracle decodes from its own cursor, so its decode of that file is what the shard has to
                   write into rows [8 * r0, ...) of the whole picture.
"""
import functools

import nosync_corpus as N

S = 128                                                   # bytes per lane
FROM_NOSYNC = ("lock_grey_910", "lock_420_130", "chain_x5", "phase_420_big")
# name -> (sampling, MCUs, seed): 63 bytes a unit, 4 / 3 / 4 units an MCU -> 72576 bytes = 567 lanes = 9 waves each
NEW = {"lock_422_288": ("422", 288, 3422), "lock_444_384": ("444", 384, 3444), "lock_440_288": ("440", 288, 3440)}
WAVES = {"lock_grey_910": 7, "lock_420_130": 6, "chain_x5": 6, "phase_420_big": 6, "lock_422_288": 9, "lock_444_384": 9, "lock_440_288": 9}
LANES = {"lock_grey_910": 448, "lock_420_130": 384, "chain_x5": 328, "lock_422_288": 567, "lock_444_384": 567, "lock_440_288": 567}
SHARD_FIXTURES = ("rstrow_200x150_444_opt", "rstrow_gray_100x60")


@functools.lru_cache(maxsize=1)
def falling():
    out = {n: N.streams()[n] for n in FROM_NOSYNC}
    for name, (sub, n_mcu, seed) in NEW.items():
        out[name] = N.lockstep(name, sub, n_mcu, seed)
    return out


def waves(stream):
    return -(-stream.n_lanes(S) // N.WAVE)


def broken():
    from test_gpu_poisoned_memory import _misplaced_restart_markers
    return _misplaced_restart_markers()


# ---- shards: file-level edits --------------------------------------------------------------------------------------------------------------
def _body(data):
    """First byte of the entropy-coded data (behind the last SOS header)."""
    sos = data.rfind(b"\xff\xda")
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


def restart_marks(data):
    """Offsets of the RSTn markers in the entropy-coded data."""
    return [i for i in range(_body(data), len(data) - 2) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def frame_height(data):
    sof = data.find(b"\xff\xc0")
    assert sof > 0
    return int.from_bytes(data[sof + 5:sof + 7], "big")


def shard_file(data, r0, r1):
    """The file that holds restart segments [r0, r1) of `data` (one segment per MCU row of 8 picture rows) and nothing else: the
    headers with the frame's height set to the shard's, the segments with their markers renumbered from RST0, an EOI."""
    body, marks = _body(data), restart_marks(data)
    nseg = len(marks) + 1
    assert 0 <= r0 < r1 <= nseg
    starts = [body] + [m + 2 for m in marks]
    ends = marks + [len(data) - 2]
    assert data[-2:] == b"\xff\xd9"
    h = frame_height(data)
    sh = h - 8 * r0 if r1 == nseg else 8 * (r1 - r0)
    sof = data.find(b"\xff\xc0")
    head = bytearray(data[:body])
    head[sof + 5:sof + 7] = sh.to_bytes(2, "big")
    out = bytes(head)
    for k, r in enumerate(range(r0, r1)):
        if k:
            out += bytes([0xFF, 0xD0 + (k - 1) % 8])
        out += data[starts[r]:ends[r]]
    return out + b"\xff\xd9", sh


class Shard:
    """Segments [r0, r1) of `data`; `file` is the shard as a picture of its own, `rows` = (first row, rows) it covers in the whole
    picture, `holds_broken`: the range contains the segment whose length was changed."""

    def __init__(self, name, data, good, r0, r1, seg):
        self.name, self.data, self.good, self.r0, self.r1 = f"{name}[{r0}:{r1}]", data, good, r0, r1
        self.file, sh = shard_file(data, r0, r1)
        self.good_file, _ = shard_file(good, r0, r1)
        self.rows = (8 * r0, sh)
        self.holds_broken = r0 <= seg < r1
        self.fixture = name


@functools.lru_cache(maxsize=1)
def shards():
    """Per fixture, of the stream with a zero byte inserted in front of the middle restart marker (segment `seg` ends late): the range
    that starts at that segment and reaches the last row, the one that starts a segment earlier, and the sibling that ends in front
    of it."""
    from conftest import golden_bytes
    out = []
    for name in SHARD_FIXTURES:
        good = golden_bytes(name)
        marks = restart_marks(good)
        seg = len(marks) // 2                              # the segment that marks[seg] ends
        m = marks[seg]
        data = good[:m] + b"\x00" + good[m:]
        assert data in broken(), name
        nseg = len(marks) + 1
        assert 8 * (nseg - 1) < frame_height(good) <= 8 * nseg, (name, "one restart segment per MCU row")
        for r0, r1 in ((seg, nseg), (seg - 1, seg + 2), (seg - 3, seg)):
            out.append(Shard(name, data, good, r0, r1, seg))
    return tuple(out)
