"""One seeded batch that takes the picture-group form (pjd_plan.cpp: 64 or more small fast pictures -> three groups by density), and the
resample requests tests/test_gpu_group_forms.py makes of it.  Host only: tests/test_group_forms_cpu.py asserts on the CPU that every
batch of the GPU file plans three groups and that every request is one its check function accepts, so a GPU case cannot pass vacuously
on the single chain or on a refused setter.

    80 small pictures   rng = default_rng(77): w in 17..97, h in 9..80; the five samplings, four qualities, dense detail on every third,
                        optimised tables on the odd ones, a restart interval of one MCU row on some 4:4:4 and grey ones
    3 larger ones       inserted after picture 30: pictures of several waves and workgroups
    2 damaged copies    of pictures 5 and 40, appended: ff 00 ff 00 in the middle of the entropy-coded data (non-zero status, partial picture)

Building it takes 0.1 s on one core."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

N_SMALL, BIG_AT, N = 80, 30, 85
DAMAGED_OF = (5, 40)                                         # small pictures k whose damaged copies stand at N - 2, N - 1
# the environment a grouped decode is planned in: every switch of the planner off (PJD_IDLE_FORM is read once per process and left alone)
ENV_OFF = ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_DC_FORM", "PJD_FORCE_SEQUENTIAL", "PJD_SUB_BYTES", "PJD_GROUPS_ALWAYS")
FILL = (114, 7, 201)
WIDTHS, HEIGHTS = (1, 5, 37, 259), (7, 9, 33)
PADS = ((0, 0, 0, 0), (2, 1, 3, 2), (0, 2, 1, 0), (5, 0, 0, 3))
FILTERS = ("bilinear", "antialias", "bicubic")
FMTS = ("rgb8", "planar", "gray")


def _synth():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    synth.build()
    return synth


def damage(j):
    """ff 00 ff 00 -- 16 one-bits, a code no table assigns -- in the middle of the entropy-coded data (tests/test_gpu_parity.py)."""
    ba = bytearray(j)
    body = bytes(ba).rfind(b"\xff\xda") + 14
    pos = body + (len(ba) - body) // 2
    while 0xFF in ba[pos - 1:pos + 5]:
        pos += 1
    ba[pos:pos + 4] = b"\xff\x00\xff\x00"
    return bytes(ba)


@functools.lru_cache(maxsize=1)
def small():
    """The 80 small pictures, in order k = 0..79."""
    synth = _synth()
    subs = [synth.SUB_420, synth.SUB_444, synth.SUB_422, synth.SUB_GREY, synth.SUB_440]
    rng = np.random.default_rng(77)
    out = []
    for k in range(N_SMALL):
        w, h = int(rng.integers(17, 98)), int(rng.integers(9, 81))
        sub = subs[k % 5]
        ri = (w + 7) // 8 if k % 7 == 3 and sub in (synth.SUB_444, synth.SUB_GREY) else 0
        out.append(synth.make(w, h, 5000 + k, (30, 60, 85, 97)[k % 4], sub, ri, synth.DENSE_DETAIL if k % 3 == 0 else 1.0, bool(k & 1)))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def jpegs():
    """The 85 streams of the batch."""
    synth = _synth()
    s = list(small())
    big = [synth.make(203, 149, 50, 95, synth.SUB_444, (203 + 7) // 8, synth.DENSE_DETAIL, True),
           synth.make(320, 240, 51, 92, synth.SUB_420, 0, synth.DENSE_DETAIL, True),
           synth.make(161, 300, 52, 75, synth.SUB_422, 0, 1.0, False)]
    out = s[:BIG_AT] + big + s[BIG_AT:] + [damage(s[k]) for k in DAMAGED_OF]
    assert len(out) == N
    return tuple(out)


@functools.lru_cache(maxsize=1)
def progressive_member():
    """(label, stream, frame) of the colour member of tests/progressive_corpus.py that case e inserts: the first 4:2:0 one of 40 x 24"""
    import progressive_corpus as PC
    for label, w in PC.corpus():
        fr = w.frame
        if (fr.width, fr.height) == (40, 24) and fr.sampling() == "420":
            return label, w.data, fr
    raise AssertionError("no 40 x 24 4:2:0 member")


def inserted(items, at):
    """items with at = {position in the result: item} inserted, lowest position first."""
    out = list(items)
    for pos in sorted(at):
        out.insert(pos, at[pos])
    return out


def scan(datas, flags=None):
    """Scanned objects (they own the memory their descriptors point into) with flags[i] OR-ed in."""
    import pjd_amd
    out = []
    for i, d in enumerate(datas):
        s = pjd_amd.Scanned(d)
        assert s.valid, i
        s.desc.flags = int(s.desc.flags) | (flags[i] if flags else 0)
        out.append(s)
    return out


def scale_cycle(n=N):
    """[(PJD_F_SCALE_* flag, s)] cycling 1, 1/2, 1/4, 1/8 per picture"""
    import pjd_amd
    c = [(0, 1), (pjd_amd.F_SCALE_1_2, 2), (pjd_amd.F_SCALE_1_4, 4), (pjd_amd.F_SCALE_1_8, 8)]
    return [c[k % 4] for k in range(n)]


def out_format(fmt):
    import pjd_amd
    return {"rgb8": pjd_amd.OUT_RGB8, "bmp": pjd_amd.OUT_BMP, "planar": pjd_amd.OUT_RGB8_PLANAR, "gray": pjd_amd.OUT_GRAY8}[fmt]


def filter_id(filt):
    import pjd_amd
    return {"bilinear": pjd_amd.RESIZE_BILINEAR, "antialias": pjd_amd.RESIZE_ANTIALIAS, "bicubic": pjd_amd.RESIZE_BICUBIC}[filt]


def groups(scanned, fmt):
    """How many picture groups the planner makes of the batch in this process' environment (0: none).  Takes the Scanned objects, not
    their descriptors: the descriptors point into memory the objects own."""
    import pjd_amd
    return pjd_amd.plan_info([s.desc for s in scanned], out_format(fmt))["dc_plan"] >> 8


# ---- the requests behind the join ------------------------------------------------------------------------------------------------------------
def resize_request(dims, filt):
    """Case b, for pictures of dims[k] = (w, h) at their decode size: per picture the content (tw, th) -- the target of Q, the resample
    before the orientation --, the window, the orientation, the pad and the delivered canvas (out_h, out_w).  Targets cycle through WIDTHS
    and HEIGHTS; where the filter refuses one (the table-driven filters take no axis more than 16x its target) the next larger of the
    list that it accepts stands in, chosen here, on the CPU, by the library's own check."""
    import pjd_amd
    req = []
    for k, (w, h) in enumerate(dims):
        win = dict(x=2, y=1, w=w - 5, h=h - 3, flags=pjd_amd.RW_HFLIP) if k % 3 == 0 else None
        o = 1 + k % 8
        pad = PADS[(k + k // 4) % 4]
        tw0, th0 = WIDTHS[k % 4], HEIGHTS[k % 3]
        cands = [(tw, th) for th in HEIGHTS if th >= th0 for tw in WIDTHS if tw >= tw0]
        tw, th = next(c for c in cands if pjd_amd.resize_window_check(w, h, c[0], c[1], win, filter_id(filt)))
        cw, ch = (th, tw) if o >= 5 else (tw, th)
        req.append(dict(target=(tw, th), win=win, o=o, pad=pad, canvas=(ch + pad[1] + pad[3], cw + pad[0] + pad[2])))
    return req


def fixed_request(dims, tw, th, filt, pad=(0, 0, 0, 0)):
    """Every picture to a content of tw x th inside `pad`, no window, orientation 1."""
    return [dict(target=(tw, th), win=None, o=1, pad=pad, canvas=(th + pad[1] + pad[3], tw + pad[0] + pad[2])) for _ in dims]


def request_ok(dims, req, filt):
    """-> the first (k, reason) the library's check functions refuse, or None"""
    import pjd_amd
    for k, ((w, h), r) in enumerate(zip(dims, req)):
        out_h, out_w = r["canvas"]
        if any(r["pad"]) and not pjd_amd.resize_pad_check(out_w, out_h, r["pad"]):
            return k, "pad"
        if not pjd_amd.resize_window_check(w, h, r["target"][0], r["target"][1], r["win"], filter_id(filt)):
            return k, "window / filter"
    return None


def warp_request(dims):
    """Case c: two views per picture in a non-monotone order, 33 x 33 and 37 x 9 in turn, a seeded similarity per view, one quarter turn
    and one view wholly outside its picture; the eight colour maps of tests/test_gpu_colour.py in turn."""
    import warp_model
    from test_gpu_colour import matrices
    n = len(dims)
    views = [(37 * k + 11) % n for k in range(n)] + list(range(n - 1, -1, -1))
    assert sorted(views) == sorted(list(range(n)) * 2)
    rng = np.random.default_rng(78)
    sizes, mats = [], []
    for v, p in enumerate(views):
        tw, th = (33, 33) if v % 2 == 0 else (37, 9)
        sizes.append((tw, th))
        mats.append(tuple(float(x) for x in warp_model.similarity(rng, dims[p][0], dims[p][1], tw, th)))
    mats[4] = (0.0, -1.0, float(dims[views[4]][0]), 1.0, 0.0, 0.0)           # a quarter turn
    mats[9] = (1.0, 0.0, 1000.0, 0.0, 1.0, -1000.0)                            # wholly outside
    cm = matrices()
    colours = [cm[v % 8] for v in range(len(views))]
    return dict(views=views, sizes=sizes, mats=mats, colours=colours)


def bound_offsets(sizes_bytes, es):
    """Byte offsets 1, 2 and 3 elements past a multiple of four elements in turn, five elements of gap between the outputs
    (tests/test_gpu_warp.py) -> (offsets, the end of the last output)."""
    offs, pos = [], 7 * es
    for i, size in enumerate(sizes_bytes):
        while (pos // es) % 4 != (i % 3) + 1:
            pos += es
        offs.append(pos)
        pos += size + 5 * es
    return offs, pos
