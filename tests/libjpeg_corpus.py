"""The seeded family PJD_F_LIBJPEG is held to beyond the committed fixtures of tests/golden/libjpeg/ (none larger than 136 x 72).
Everything is encoded by tools/synth.py from fixed seeds in well under two seconds a picture; nothing here decodes on a device and
nothing is committed.

    small(sampling)     [(name, jpeg)]  the 180 pictures W = 1..20 x H = 1..9 of one sampling: every W % 4 with fancy upsampling on
                        (n = ceil(W/2) >= 3) and off, n == 3 with the special last column inside (W = 6) and outside (W = 5) the
                        picture, one and two chroma rows (m = 1, 2: the neighbour row clamped to itself), one and two MCUs each way
    edges()             [(name, jpeg)]  widths one to three past a multiple of 256 and of 4 in every sampling (the tail store of the
                        colour kernel, more than one workgroup of it, several back-end ranges), restart markers, pictures of 0 / 255
                        noise at low and high quality (the IDCT's clamp and the three colour clamps), and the smallest pictures with
                        fancy upsampling on, W % 4 in {2, 3} and m = 1
    limits()            [(name, jpeg)]  strips with an axis of 65497..65500 (libjpeg's own limit is 65500: Pillow still decodes them)
                        and the members of tests/geometry_corpus.py in a sampling the flag takes (an axis of 65535: beyond libjpeg, the
                        model alone is the expectation there)
    model_bytes(name)   the bytes whose coefficients the model reads: the member's own, but for a subsampled member with DRI, where
                        the oracle port follows the reference's restart rule -- there the same picture encoded without DRI (the
                        flag implies the T.81 rule, under which both files hold the same coefficients)
    expected(port, data) -> (status, H x W x 3 picture): tests/libjpeg_model.py over the oracle port's coefficients under the T.81
                        zigzag; the status is the port's, a broken stream gives the partial picture
    dims(name)          (w, h, sampling)

Left out of limits(): the 4:4:0 members (outside the mode's envelope), `h16x65535_420_ri1_ref` (the flag implies the T.81 restart
rule: it is its `_std` twin), and `segs_65535x72_444_ri1` and `dri65535_65535x72_444` (4.7 MPix each: oracle port and model together
need more than a few seconds on them, and 65535 x 8 with and without DRI 1 is in).
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import geometry_corpus as G      # noqa: E402
import libjpeg_model as M        # noqa: E402
import synth                     # noqa: E402

S444, S422, S420, GREY = synth.SUB_444, synth.SUB_422, synth.SUB_420, synth.SUB_GREY
SAMPLINGS = {"444": S444, "422": S422, "420": S420, "grey": GREY}
LUMA = {S444: (1, 1), S422: (2, 1), S420: (2, 2), GREY: (1, 1)}      # luma (h, v)
SMALL_W, SMALL_H = range(1, 21), range(1, 10)

# name -> (w, h, sampling, quality, DRI, seed)
EDGES = {
    "e259x37_420": (259, 37, S420, 85, 0, 9501),
    "e515x21_422": (515, 21, S422, 85, 0, 9502),
    "e1030x9_444": (1030, 9, S444, 85, 0, 9503),
    "e257x19_grey": (257, 19, GREY, 85, 0, 9504),
    "e2049x17_420": (2049, 17, S420, 85, 0, 9505),
    "e301x203_420_q30": (301, 203, S420, 30, 0, 9506),
    "e200x150_444_ri25": (200, 150, S444, 85, 25, 9507),
    # the smallest pictures with fancy upsampling on, W % 4 in {2, 3}, and with one chroma row
    "e6x3_420": (6, 3, S420, 90, 0, 9508),
    "e7x2_420": (7, 2, S420, 90, 0, 9509),
    "e10x1_420": (10, 1, S420, 90, 0, 9510),
    "e6x1_422": (6, 1, S422, 90, 0, 9511),
    "e11x2_422": (11, 2, S422, 90, 0, 9512),
}
# pictures of 0 / 255 noise: name -> (w, h, sampling, quality, seed)
SATURATING = {
    "sat67x35_420_q100": (67, 35, S420, 100, 9601),
    "sat67x35_444_q30": (67, 35, S444, 30, 9602),
    "sat259x19_422_q10": (259, 19, S422, 10, 9603),
    "sat130x40_420_q5": (130, 40, S420, 5, 9604),
}
# an axis of 65497..65500, and a width just past 32768: name -> (w, h, sampling, quality, DRI, seed)
LIMITS_65500 = {
    "l65500x16_420": (65500, 16, S420, 85, 0, 9701),
    "l65499x9_422": (65499, 9, S422, 85, 0, 9702),
    "l16x65500_420": (16, 65500, S420, 85, 0, 9703),
    "l9x65499_422": (9, 65499, S422, 85, 0, 9704),
    "l3x65500_420": (3, 65500, S420, 85, 0, 9705),
    "l32769x8_444": (32769, 8, S444, 85, 0, 9706),
    "l65497x17_420_ri1": (65497, 17, S420, 85, 1, 9707),
}
LEFT_OUT = ["h1x65535_440", "w32769x17_440", G.REF_RULE] + G.BIG
GEOMETRY = [n for n in G.NAMES if n not in LEFT_OUT]      # an axis of 65535 (and 65529, 32768): beyond what libjpeg decodes
WIDE_420 = "w65535x16_420"


def small_name(w, h, tag):
    return f"s{w}x{h}_{tag}"


@functools.lru_cache(maxsize=None)
def _make(w, h, seed, quality, sub, ri):
    return synth.make(w, h, seed, quality, sub, ri)


@functools.lru_cache(maxsize=None)
def _saturating(name):
    w, h, sub, quality, seed = SATURATING[name]
    rgb = (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return synth.encode(rgb, quality, sub)


def _small_spec(w, h, tag):
    return w, h, SAMPLINGS[tag], (30, 90, 100)[(w + h) % 3], 0, 9000 + 16 * w + h


def _spec(name):
    """(w, h, sampling, quality, DRI, seed) of a member made by synth.make"""
    if name in EDGES:
        return EDGES[name]
    if name in LIMITS_65500:
        return LIMITS_65500[name]
    if name in G.MEMBERS:
        w, h, sub, ri, seed, _ = G.MEMBERS[name]
        return w, h, sub, 85, ri, seed
    size, tag = name[1:].split("_")
    w, h = (int(v) for v in size.split("x"))
    return _small_spec(w, h, tag)


def dims(name):
    if name in SATURATING:
        return SATURATING[name][:3]
    return _spec(name)[:3]


def jpeg(name):
    if name in SATURATING:
        return _saturating(name)
    w, h, sub, quality, ri, seed = _spec(name)
    return _make(w, h, seed, quality, sub, ri)


def model_bytes(name):
    if name in SATURATING:
        return _saturating(name)
    w, h, sub, quality, ri, seed = _spec(name)
    return _make(w, h, seed, quality, sub, 0 if LUMA[sub] != (1, 1) else ri)


def small(tag):
    """[(name, jpeg)] of one sampling: "444", "422", "420" or "grey" """
    return [(small_name(w, h, tag), jpeg(small_name(w, h, tag))) for w in SMALL_W for h in SMALL_H]


def edges():
    return [(n, jpeg(n)) for n in list(EDGES) + list(SATURATING)]


def limits():
    return [(n, jpeg(n)) for n in list(LIMITS_65500) + GEOMETRY]


def pillow_decodes(name):
    """libjpeg refuses a dimension above 65500"""
    w, h, _ = dims(name)
    return max(w, h) <= 65500


# ---- the model, with its two loops over units and rows written on whole arrays (held equal to libjpeg_model's on the small family) -----
def unit_grids(coef, width, height, ncomp, hs, vs):
    """libjpeg_model.unit_grids"""
    flat = np.asarray(coef, np.int16).reshape(-1)
    w8, h8 = (width + 7) // 8, (height + 7) // 8
    wr = w8 + (1 if hs == 2 and w8 % 2 else 0)
    mcux, mcuy = (w8 + hs - 1) // hs, (h8 + vs - 1) // vs
    flat = np.concatenate([flat, np.zeros(64, np.int16)])      # a unit the buffer does not hold reads as zeros
    nowhere = flat.size - 64

    def gather(comp, ys, xs):
        y, x = np.meshgrid(np.asarray(ys, np.int64), np.asarray(xs, np.int64), indexing="ij")
        blk = (y // 2) * ((wr + 1) // 2) + x // 2
        o = blk * 768 + comp * 256 + ((y % 2) * 2 + x % 2) * 64
        o = np.where(o + 64 <= nowhere, o, nowhere)
        return flat[o[..., None] + np.arange(64)]

    grids = [gather(0, np.arange(mcuy * vs), np.arange(mcux * hs))]
    for c in range(1, ncomp):
        grids.append(gather(c, np.arange(mcuy) * vs, np.arange(mcux) * hs))
    return grids


def upsample(c, width, height, hs, vs):
    """libjpeg_model.upsample"""
    if hs == 1 and vs == 1:
        return c[:height, :width]
    assert hs == 2
    n, m = (width + 1) // 2, (height + vs - 1) // vs
    c = c[:m, :n].astype(np.int64)
    y = np.arange(height)
    r = y // vs
    if n <= 2:
        return np.repeat(c[r], 2, axis=1)[:, :width].astype(np.uint8)
    prev, nxt = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.zeros((height, 2 * n), np.int64)
    if vs == 1:
        out[:, 0::2] = ((3 * c + prev + 1) >> 2)[r]
        out[:, 1::2] = ((3 * c + nxt + 2) >> 2)[r]
        out[:, 0], out[:, 2 * n - 1] = c[r, 0], c[r, n - 1]
    else:
        nb = np.where(y % 2 == 0, np.maximum(r - 1, 0), np.minimum(r + 1, m - 1))
        s = 3 * c[r] + c[nb]
        sp, sn = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[:, 0::2] = (3 * s + sp + 8) >> 4
        out[:, 1::2] = (3 * s + sn + 7) >> 4
    return out[:, :width].astype(np.uint8)


def decode(coef, qts, width, height, ncomp, hs, vs):
    """libjpeg_model.decode over the two array forms above"""
    grids = unit_grids(coef, width, height, ncomp, hs, vs)
    planes = [M.plane_from_units(M.idct_units(g, np.asarray(qts[c]).reshape(64))) for c, g in enumerate(grids)]
    yp = planes[0][:height, :width]
    if ncomp == 1:
        return np.stack([yp, yp, yp], axis=-1)
    return M.ycc_to_rgb(yp, upsample(planes[1], width, height, hs, vs), upsample(planes[2], width, height, hs, vs))


def port_coefficients(port, data):
    """The oracle port's entropy decode under the T.81 zigzag: (status, coefficients, the model's other arguments)"""
    port.standard_zigzag(True)
    try:
        d = port.decode(data)
    finally:
        port.standard_zigzag(False)
    assert d["valid"]
    info = d["info"]
    qts = [info["qt"][info["comp_qt"][k]] for k in range(info["ncomp"])]
    return d["huff_rc"], d["coef"], (qts, info["width"], info["height"], info["ncomp"], info["hsamp"], info["vsamp"])


def expected(port, data):
    """(status, picture) of a flagged descriptor of `data`: a broken stream gives the port's status and the partial picture"""
    status, coef, args = port_coefficients(port, data)
    return status, decode(coef, *args)


def entropy_cut(data, fraction):
    """geometry_corpus.truncated's rule on any stream: `fraction` of the entropy-coded bytes, then an EOI; not behind a 0xFF"""
    lo, hi = G.entropy_span(data)
    cut = lo + int((hi - lo) * fraction)
    while data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + b"\xff\xd9"
