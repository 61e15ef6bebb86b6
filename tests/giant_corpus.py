"""Pictures at the SIZE limits: 1.6 GPix pictures whose output passes 4 GiB inside one picture, canvas or plane, and a stream of
2^29 - 1 entropy-coded bytes, the most the planner takes.  None of them is encoded or decoded whole on the CPU.

tools/synth.py encodes a PERIOD picture of W x (8 MCU rows) whose DRI is one MCU row, so it has 8 restart segments.  Its entropy-coded
bytes are cut at RST0..RST6 into 8 segment bodies, and the giant's stream is body[r % 8] for r = 0, 1, ... with RST((r - 1) % 8)
between them, behind the period's headers with the SOF height patched.  Every segment resets the DC predictors, the reference's chroma
upsampling is nearest-neighbour inside an MCU and libjpeg's h2v1 upsampling is horizontal, so the giant's expected picture is the
period's expected picture tiled vertically and cut at H (tests/test_giant_cpu.py holds that at 203 x 213 against whole decodes).  So
that the picture is not purely periodic, the segments of marks() come from a second period picture with another seed: the first and
the last, and those around every row in which a byte offset of one of the member's output formats passes a multiple of 2^32.

    jpeg(name)                         the member's bytes
    splice(period_jpeg, H, marks=(), alt_jpeg=None, pad_to=None, last_body=None)
    marks(name)                        sorted segment indices that come from the second period
    crossings(name)                    {format: [rows holding the byte before / at a multiple of 2^32]}
    expected_rows(name, y0, y1, ...)   rows y0..y1 of the expected picture, from the two period expectations alone
    period_expected(name, ...)         (main, alt) period expectations, H_period x W x 3 (H_period x W for grey)

This module imports no library of the project; nothing is committed under golden/.
"""
import functools
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import synth      # noqa: E402

F_STANDARD_RESTART, F_LIBJPEG = 1, 64      # pjd_amd.F_* (this module imports no library)
S444, S422, S420 = synth.SUB_444, synth.SUB_422, synth.SUB_420
LUMA = {S444: (1, 1), S422: (2, 1), S420: (2, 2)}      # luma (h, v)
TWO32 = 1 << 32
ECS_CAP = (1 << 29) - 1      # the longest stream the planner takes (include/pjd.h)
ALT = 50                     # seed of the second period = seed + ALT

# name -> (W, H, sampling, quality, detail, seed, flags the member may be decoded under, formats it is decoded in)
# H None: computed (full_height()).  The DRI is one MCU row: 8192, 4096 and 1366 MCUs.
MEMBERS = {
    "g444": (65535, 24571, S444, 30, 0.25, 7101, (0,), ("rgb8", "planar", "gray", "bmp")),
    "g420_std": (65535, 24571, S420, 30, 0.25, 7102, (F_STANDARD_RESTART,), ("rgb8", "planar")),
    "g422_tall": (21851, 65535, S422, 30, 0.25, 7103, (F_STANDARD_RESTART, F_LIBJPEG), ("rgb8", "planar", "gray")),
    "g444_full": (65535, None, S444, 85, 1.0, 7104, (0,), ("rgb8",)),
}
FULL, FULL_ERR = "g444_full", "g444_full_err"
NAMES = list(MEMBERS)
ERR_CODE = b"\xff\x00\xff\x00"      # 16 one-bits, destuffed: a code no table assigns (tests/stream_cases.py)


def _base(name):
    return FULL if name == FULL_ERR else name


def spec(name):
    return MEMBERS[_base(name)]


def seg_rows(sub):
    """picture rows of one restart segment (one MCU row)"""
    return 8 * LUMA[sub][1]


def period_dims(name):
    w, _, sub = spec(name)[:3]
    return w, 8 * seg_rows(sub)


def dri(name):
    w, _, sub = spec(name)[:3]
    return -(-w // (8 * LUMA[sub][0]))


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def entropy_span(data):
    """(first, last + 1) of the entropy-coded bytes: after the SOS header, before the EOI"""
    sos = data.rfind(b"\xff\xda")
    body = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    assert data[-2:] == b"\xff\xd9"
    return body, len(data) - 2


def bodies(period_jpeg):
    """the 8 segment bodies of a period picture, restart markers removed (they must be RST0..RST6 in order)"""
    lo, hi = entropy_span(period_jpeg)
    ecs = period_jpeg[lo:hi]
    found = re.findall(rb"\xff[\xd0-\xd7]", ecs)
    assert found == [bytes([0xFF, 0xD0 + k]) for k in range(7)], "a period picture has 8 restart segments"
    out = re.split(rb"\xff[\xd0-\xd7]", ecs)
    assert len(out) == 8
    return out


def destuffed_len(body):
    """what the scanner counts: a stuffed 0xFF 0x00 is one byte"""
    return len(body) - body.count(b"\xff\x00")


def patched_headers(period_jpeg, height):
    """the period's bytes up to the entropy-coded data, with the SOF0 height replaced"""
    lo, _ = entropy_span(period_jpeg)
    head = bytearray(period_jpeg[:lo])
    i = 2
    while i < lo:
        assert head[i] == 0xFF
        marker, length = head[i + 1], (head[i + 2] << 8) | head[i + 3]
        if marker == 0xC0:
            head[i + 5], head[i + 6] = height >> 8, height & 0xFF
            return bytes(head)
        i += 2 + length
    raise AssertionError("no SOF0")


def splice(period_jpeg, height, marks=(), alt_jpeg=None, pad_to=None, last_body=None):
    """The giant of `height` rows: segment r is body[r % 8] of the period, of `alt_jpeg` where r is in marks; last_body replaces the last
    segment's; pad_to: zero bytes before the EOI until the destuffed stream holds that many bytes."""
    main = bodies(period_jpeg)
    alt = bodies(alt_jpeg) if alt_jpeg is not None else None
    rows = _seg_rows_of(period_jpeg)
    n = -(-height // rows)
    marks = set(marks)
    assert not marks or alt is not None
    parts = [patched_headers(period_jpeg, height)]
    total = 0
    for r in range(n):
        if r:
            parts.append(bytes([0xFF, 0xD0 + (r - 1) % 8]))
        b = (alt if r in marks else main)[r % 8]
        if r == n - 1 and last_body is not None:
            b = last_body
        parts.append(b)
        total += destuffed_len(b) if pad_to is not None else 0
    if pad_to is not None:
        assert total <= pad_to, (total, pad_to)
        parts.append(bytes(pad_to - total))
    parts.append(b"\xff\xd9")
    return b"".join(parts)


def _seg_rows_of(jpeg_bytes):
    """8 x the luma vertical sampling factor, read from the SOF0 header"""
    i = 2
    while True:
        assert jpeg_bytes[i] == 0xFF
        marker, length = jpeg_bytes[i + 1], (jpeg_bytes[i + 2] << 8) | jpeg_bytes[i + 3]
        if marker == 0xC0:
            return 8 * (jpeg_bytes[i + 11] & 15)      # component 1's sampling byte: h << 4 | v
        i += 2 + length


@functools.lru_cache(maxsize=None)
def period_jpeg(name, alt=False, with_dri=True):
    """the (second) period picture of a member; with_dri False: the same picture encoded without restart markers"""
    w, _, sub, quality, detail, seed, _, _ = spec(name)
    pw, ph = period_dims(name)
    return synth.make(pw, ph, seed + (ALT if alt else 0), quality, sub, dri(name) if with_dri else 0, detail)


# ---- where offsets pass 2^32 -----------------------------------------------------------------------------------------------------------
def row_offsets(w, h, fmt):
    """[(first byte, bytes) of every picture row y, per plane] of one picture of w x h in `fmt`, from the picture's first byte"""
    y = np.arange(h, dtype=np.int64)
    if fmt == "rgb8":
        return [(y * (3 * w), 3 * w)]
    if fmt == "bmp":
        stride = 3 * w + w % 4
        return [(26 + (h - 1 - y) * stride, stride)]
    if fmt == "planar":
        return [(c * w * h + y * w, w) for c in range(3)]
    if fmt == "gray":
        return [(y * w, w)]
    raise ValueError(fmt)


def out_bytes(w, h, fmt):
    return {"rgb8": 3 * w * h, "bmp": 26 + h * (3 * w + w % 4), "planar": 3 * w * h, "gray": w * h}[fmt]


def _crossings_of(w, h, fmt):
    rows = set()
    for first, n in row_offsets(w, h, fmt):
        for m in range(TWO32, out_bytes(w, h, fmt), TWO32):
            for byte in (m - 1, m):
                hit = np.flatnonzero((first <= byte) & (byte < first + n))
                rows.update(int(v) for v in hit)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def height(name):
    h = spec(name)[1]
    return h if h is not None else full_height()


def crossings(name):
    w, _, _, _, _, _, _, formats = spec(name)
    return {f: _crossings_of(w, height(name), f) for f in formats}


def _marks_for(w, h, sub, formats):
    """The first and the last segment, and around every crossing row its own segment and the neighbour on the side the row lies nearer
    to (the row before a crossing between two rows and the row after it are both in: "both segments that touch the row")."""
    rows_per = seg_rows(sub)
    n = -(-h // rows_per)
    out = {0, n - 1}
    for f in formats:
        for y in _crossings_of(w, h, f):
            s = y // rows_per
            out.add(s)
            out.add(min(n - 1, s + 1) if (y % rows_per) * 2 >= rows_per else max(0, s - 1))
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def marks(name):
    w, _, sub, _, _, _, _, formats = spec(name)
    return _marks_for(w, height(name), sub, formats)


@functools.lru_cache(maxsize=None)
def n_segments(name):
    return -(-height(name) // seg_rows(spec(name)[2]))


# ---- the stream-limit member -----------------------------------------------------------------------------------------------------------
def _stream_len(n, main_len, alt_len, w, sub, formats):
    mk = set(_marks_for(w, n * seg_rows(sub), sub, formats))
    return sum((alt_len if r in mk else main_len)[r % 8] for r in range(n))


@functools.lru_cache(maxsize=1)
def full_height():
    """The largest height at which the destuffed stream of g444_full stays below 2^29 - 1 (the marks depend on the height, so the
    search recounts them); a multiple of 8, since the stream depends on the number of MCU rows alone."""
    w, _, sub, _, _, _, _, formats = MEMBERS[FULL]
    main_len = [destuffed_len(b) for b in bodies(period_jpeg(FULL))]
    alt_len = [destuffed_len(b) for b in bodies(period_jpeg(FULL, alt=True))]
    n = ECS_CAP // (max(sum(main_len), sum(alt_len)) // 8 + 1) - 16
    assert _stream_len(n, main_len, alt_len, w, sub, formats) < ECS_CAP
    while n < 8192 and _stream_len(n + 1, main_len, alt_len, w, sub, formats) < ECS_CAP:
        n += 1
    assert n < 8192, "the stream never reaches the cap"
    return 8 * n


def file_positions(body):
    """file offset in `body` of every destuffed byte"""
    pos, i = [], 0
    while i < len(body):
        pos.append(i)
        i += 2 if body[i] == 0xFF else 1
    return pos


def damaged_body(body, back):
    """`body` with ERR_CODE over the four file bytes that begin `back` destuffed bytes before its end; None where a 0xFF is near"""
    f = file_positions(body)[-back]
    if f + 4 > len(body) or 0xFF in body[f - 1:f + 5]:
        return None
    return body[:f] + ERR_CODE + body[f + 4:]


def period_variant(name, slot, body):
    """the second period picture with the body of segment `slot` replaced"""
    alt = period_jpeg(name, alt=True)
    bs = bodies(alt)
    bs[slot] = body
    lo, _ = entropy_span(alt)
    parts = [alt[:lo]]
    for k, b in enumerate(bs):
        if k:
            parts.append(bytes([0xFF, 0xD0 + k - 1]))
        parts.append(b)
    return b"".join(parts) + b"\xff\xd9"


def _y_units(port, data):
    """(status, the Y units as a grid rows x columns x 64) of the port's entropy decode"""
    d = port.decode(data)
    assert d["valid"]
    info = d["info"]
    flat = np.concatenate([d["coef"].reshape(-1), np.zeros(64, np.int16)])
    w8, h8 = (info["width"] + 7) // 8, (info["height"] + 7) // 8
    y, x = np.meshgrid(np.arange(h8, dtype=np.int64), np.arange(w8, dtype=np.int64), indexing="ij")
    o = ((y // 2) * ((w8 + 1) // 2) + x // 2) * 768 + ((y % 2) * 2 + x % 2) * 64
    o = np.where(o + 64 <= flat.size - 64, o, flat.size - 64)
    return d["huff_rc"], flat[o[..., None] + np.arange(64)], d


@functools.lru_cache(maxsize=1)
def full_err_damage():
    """(slot, damaged body, period variant, its port decode): the erring code planted as near the end of the last segment as makes the
    port report an error whose first changed unit lies in the segment's last MCU."""
    port = _port()
    n = n_segments(FULL)
    slot = (n - 1) % 8
    assert (n - 1) in marks(FULL)
    good = bodies(period_jpeg(FULL, alt=True))[slot]
    _, units_good, _ = _y_units(port, period_jpeg(FULL, alt=True))
    last = units_good.shape[1] - 1
    for back in range(4, 40):
        bad = damaged_body(good, back)
        if bad is None:
            continue
        variant = period_variant(FULL, slot, bad)
        status, units, d = _y_units(port, variant)
        if status == 0:
            continue
        diff = (units != units_good).any(axis=-1)
        if diff[:slot].any() or diff[slot, :last].any():
            break                                            # the plant reaches back into an earlier MCU: none nearer the end erred
        # the error must be the planted code itself, whatever follows the segment: the same segment as the LAST of a picture, zero
        # bytes behind it as in the giant, gives the same status and the same rows
        alt = period_jpeg(FULL, alt=True)
        ends = splice(alt, 8 * (slot + 1), pad_to=sum(destuffed_len(b) for b in bodies(alt)[:slot]) + destuffed_len(bad) + 4096, last_body=bad)
        e = port.decode(ends)
        if e["huff_rc"] != status or not np.array_equal(e["rgb"][8 * slot:], d["rgb"][8 * slot:8 * slot + 8]):
            continue
        return slot, bad, variant, d
    raise AssertionError("no placement of the erring code in the last MCU")


@functools.lru_cache(maxsize=None)
def jpeg(name):
    w, _, sub = spec(name)[:3]
    h = height(name)
    main, alt = period_jpeg(name), period_jpeg(name, alt=True)
    if name == FULL:
        return splice(main, h, marks(name), alt, pad_to=ECS_CAP)
    if name == FULL_ERR:
        return splice(main, h, marks(name), alt, pad_to=ECS_CAP, last_body=full_err_damage()[1])
    return splice(main, h, marks(name), alt)


# ---- expectations ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _port():
    import oracle_lib
    return oracle_lib.Port()


def expected_picture(port, data_dri, data_plain, sub, flags, gray=False):
    """(status, picture) a descriptor of `data_dri` under `flags` is expected to decode to: the oracle port's decode under the
    reference's arithmetic -- of the same picture encoded without DRI (`data_plain`) where the standard restart rule applies to a
    subsampled picture, as geometry_corpus.oracle_bytes --, libjpeg_corpus.expected under F_LIBJPEG, gray_expected's planes for grey."""
    import gray_expected
    import libjpeg_corpus
    subsampled = LUMA[sub] != (1, 1)
    if flags & F_LIBJPEG:
        data = data_plain if subsampled else data_dri
        if gray:
            return gray_expected.model_y_plane(port, data, broken=True)
        return libjpeg_corpus.expected(port, data)
    data = data_plain if (subsampled and flags & F_STANDARD_RESTART) else data_dri
    if gray:
        return gray_expected.ref_plane(port, data)
    d = port.decode(data)
    assert d["valid"]
    return d["huff_rc"], d["rgb"]


@functools.lru_cache(maxsize=None)
def period_expected(name, flags=None, gray=False):
    """(main, alt): the expected pictures of the two period pictures of a member, read-only"""
    sub, member_flags = spec(name)[2], spec(name)[6]
    flags = member_flags[0] if flags is None else flags
    assert flags in member_flags, (name, flags)
    out = []
    for alt in (False, True):
        status, pic = expected_picture(_port(), period_jpeg(name, alt), period_jpeg(name, alt, with_dri=False), sub, flags, gray)
        assert status == 0, (name, alt, status)
        pic = np.ascontiguousarray(pic)
        pic.setflags(write=False)
        out.append(pic)
    return tuple(out)


@functools.lru_cache(maxsize=1)
def full_err_expected():
    """(status, the rows of the last segment) of g444_full_err: the port's for the period variant carrying the same damage"""
    slot, _, _, d = full_err_damage()
    rows = np.ascontiguousarray(d["rgb"][8 * slot:8 * slot + 8])
    rows.setflags(write=False)
    return d["huff_rc"], rows


def expected_rows(name, y0, y1, flags=None, gray=False):
    """Rows y0 <= y < y1 of the expected picture (y1 - y0 x W x 3; y1 - y0 x W for grey), from the period expectations alone."""
    h, per = height(name), seg_rows(spec(name)[2])
    assert 0 <= y0 <= y1 <= h
    main, alt = period_expected(_base(name), flags, gray)
    last = None
    if name == FULL_ERR:
        assert not gray
        last = (n_segments(name) - 1, full_err_expected()[1])
    return tile(main, alt, marks(name), per, y0, y1, last)


def tile(main, alt, marks, per, y0, y1, last=None):
    """Rows y0 <= y < y1 of the picture whose segment r (of `per` rows) is segment r % 8 of `main`, of `alt` where r is in marks;
    last = (segment, its rows) replaces one segment."""
    mk = set(marks)
    out = np.empty((y1 - y0,) + main.shape[1:], np.uint8)
    y = y0
    while y < y1:
        r = y // per
        top = min(y1, (r + 1) * per)
        if last is not None and r == last[0]:
            rows = last[1][y % per:y % per + top - y]
        else:
            lo = (r % 8) * per + y % per
            rows = (alt if r in mk else main)[lo:lo + top - y]
        out[y - y0:top - y0] = rows
        y = top
    return out
