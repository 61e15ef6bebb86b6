"""Pictures at the dimension limits: strips 65535 samples long on one axis and one or a few MCUs on the other, in every sampling,
widths on both sides of 32768 (where the resize taps change from 32-bit to 64-bit arithmetic), one MCU column thousands of MCU rows
tall, restart intervals of one MCU by the thousand (more than 2^16 segments in one picture) and a DRI of 65535.  Everything is encoded
by tools/synth.py from fixed seeds in well under two seconds a picture; nothing here decodes and nothing is committed.

    family()            [(name, jpeg, flags)]     the members, in an order that localises a failure (widths, heights, 32768, segments)
    oracle_bytes(name)  the bytes whose oracle decode is the member's expected picture (the member's own, but for the `_std` member)
    truncated(name)     the member cut to half of its entropy-coded bytes, headers and an EOI kept
    geometry(name)      (w, h, sub, ri) of a member
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import synth      # noqa: E402

F_STANDARD_RESTART = 1      # pjd_amd.F_STANDARD_RESTART (this module imports no library)

S444, S422, S420, S440, GREY = synth.SUB_444, synth.SUB_422, synth.SUB_420, synth.SUB_440, synth.SUB_GREY

# name -> (w, h, sampling, DRI, seed, flags)
MEMBERS = {
    "w65535x8_444": (65535, 8, S444, 0, 6101, 0),
    "w65535x16_420": (65535, 16, S420, 0, 6102, 0),                  # the last MCU holds 15 of 16 columns
    "w65535x9_422": (65535, 9, S422, 0, 6103, 0),                    # the second MCU row holds one picture row
    "w65535x1_grey": (65535, 1, GREY, 0, 6104, 0),
    "w65529x8_444_ri1": (65529, 8, S444, 1, 6105, 0),                # 8192 segments; one pixel into the last MCU
    "h8x65535_444_ri1": (8, 65535, S444, 1, 6106, 0),                # 8192 segments; mcux == 1
    "h16x65535_420": (16, 65535, S420, 0, 6107, 0),
    "h1x65535_440": (1, 65535, S440, 0, 6108, 0),
    "h9x65535_422": (9, 65535, S422, 0, 6109, 0),
    "w32768x8_444": (32768, 8, S444, 0, 6110, 0),
    "w32769x17_440": (32769, 17, S440, 0, 6111, 0),
    "segs_65535x72_444_ri1": (65535, 72, S444, 1, 6112, 0),          # 73728 segments: more than 2^16
    "dri65535_65535x72_444": (65535, 72, S444, 65535, 6113, 0),      # two segments; the second starts in the middle of MCU row 7
    "h16x65535_420_ri1_std": (16, 65535, S420, 1, 6114, F_STANDARD_RESTART),
    "h16x65535_420_ri1_ref": (16, 65535, S420, 1, 6114, 0),          # the same bytes under the reference's restart rule
}
NAMES = list(MEMBERS)
REF_RULE = "h16x65535_420_ri1_ref"      # the one member the planner routes to the exact kernel
STD_RULE = "h16x65535_420_ri1_std"
RI1 = ["w65529x8_444_ri1", "h8x65535_444_ri1", "segs_65535x72_444_ri1"]
DRI65535 = "dri65535_65535x72_444"
BIG = ["segs_65535x72_444_ri1", DRI65535]      # the two 4.7 MPix members
SAMPLING = {S444: (1, 1), S422: (2, 1), S420: (2, 2), S440: (1, 2), GREY: (1, 1)}      # luma (h, v)


def geometry(name):
    w, h, sub, ri, _, _ = MEMBERS[name]
    return w, h, sub, ri


def n_mcu(name):
    w, h, sub, _ = geometry(name)
    hs, vs = SAMPLING[sub]
    return (-(-w // (8 * hs))) * (-(-h // (8 * vs)))


def n_segments(name):
    """ceil(n_mcu / DRI), one without DRI."""
    ri = geometry(name)[3]
    return -(-n_mcu(name) // ri) if ri else 1


@functools.lru_cache(maxsize=None)
def _make(w, h, seed, sub, ri):
    return synth.make(w, h, seed, 85, sub, ri)


@functools.lru_cache(maxsize=1)
def family():
    """[(name, jpeg_bytes, flags)]"""
    return [(n, _make(w, h, seed, sub, ri), flags) for n, (w, h, sub, ri, seed, flags) in MEMBERS.items()]


def jpeg(name):
    w, h, sub, ri, seed, _ = MEMBERS[name]
    return _make(w, h, seed, sub, ri)


def flags(name):
    return MEMBERS[name][5]


def oracle_bytes(name):
    """What the oracle decodes for the member's expected picture.  Under PJD_F_STANDARD_RESTART a subsampled picture with DRI is the
    picture encoded without DRI (the oracle follows the reference's own rule, which garbles it); every other member is its own."""
    w, h, sub, ri, seed, fl = MEMBERS[name]
    return _make(w, h, seed, sub, 0 if fl & F_STANDARD_RESTART else ri)


def entropy_span(data):
    """(first, last + 1) of the entropy-coded bytes: after the SOS header, before the EOI."""
    sos = data.rfind(b"\xff\xda")
    body = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    assert data[-2:] == b"\xff\xd9"
    return body, len(data) - 2


@functools.lru_cache(maxsize=None)
def truncated(name, fraction=0.5):
    """The member with `fraction` of its entropy-coded bytes, then an EOI.  The cut does not fall behind a 0xFF (a stuffed byte or a
    restart marker stays whole), so the scanner accepts the file; what the decoder reports is the oracle's business."""
    data = jpeg(name)
    lo, hi = entropy_span(data)
    cut = lo + int((hi - lo) * fraction)
    while data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + b"\xff\xd9"
