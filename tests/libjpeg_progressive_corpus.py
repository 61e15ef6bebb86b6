"""What PJD_F_LIBJPEG is held to on progressive (SOF2) frames; host only, nothing here decodes on a device.

    fixtures()              [(name, jpeg, frame, manifest case)]  the committed members of tests/golden/libjpeg_progressive/: Pillow's
                            coefficients rewritten under hand-made COMPLETE scan scripts; record(name) is Pillow's decode of each
    model_expected(data, frame) -> (status, coefficients in the download's layout, RGB picture, luma plane): tests/libjpeg_model.py over
                            the coefficients of the bit-level model of tests/jpeg_progressive.py -- for a broken stream the
                            coefficients stored up to the error, and their picture
    corpus_items()          [(label, jpeg, frame)]  the 46 members of progressive_corpus.corpus() the flag takes
    refused_items()         the 9 members that are 4:4:0
    broken_items()          every ninth stream of progressive_corpus.broken() and the two of desynchronised()
    edge_items()            jpeg_progressive.edge_streams: stores that truncate to -32768, which in a progressive frame is a value

A complete member is held to libjpeg itself (the recorded Pillow decode).  The corpus is not: about half of it differs from Pillow,
because its coefficients reach +-1023 under quantisers up to 40 -- the overflow region include/pjd.h assigns to pjd_libjpeg_idct --
and because libjpeg smooths a frame whose scans leave coefficients unrefined.  There the expectation is the model.
"""
import functools
import hashlib
import json
import os

import numpy as np

import jpeg_progressive as P
import jpeg_symbols as J
import libjpeg_model as M
import progressive_corpus as PC
import symbol_corpus as SC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "libjpeg_progressive")
SAMPLING_NAMES = {"grey": "grey", "444": "4:4:4", "422": "4:2:2", "420": "4:2:0", "440": "4:4:0"}


def frame_of_jpeg(data):
    """The Frame of a SOF2 file: its size, sampling factors and the DQT entries in the order the file holds them (zigzag), decoded with
    T.81's map.  The Huffman tables of the Frame serve only its baseline twin (progressive_corpus.twin)."""
    p, qt, qt16 = 2, {}, set()
    while True:
        assert data[p] == 0xFF
        m, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + ln]
        p += 2 + ln
        if m == 0xDB:
            q = 0
            while q < len(seg):
                wide, t = seg[q] >> 4, seg[q] & 15
                n = 128 if wide else 64
                body = seg[q + 1:q + 1 + n]
                qt[t] = [(body[2 * k] << 8) | body[2 * k + 1] for k in range(64)] if wide else list(body)
                if wide:
                    qt16.add(t)
                q += 1 + n
        elif m == 0xC2:
            height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [J.Component(seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k], 0, 0) for k in range(seg[5])]
            break
        else:
            assert m not in (0xC0, 0xC1, 0xDA), "a progressive file is expected"
    used = {c.tq for c in comps}
    fr = J.Frame(width, height, comps, {0: SC.dc_general()}, {0: SC.ac_162()}, qt={t: qt[t] for t in sorted(used)}, qt16=qt16 & used)
    fr.standard_zigzag = True
    return fr


@functools.lru_cache(maxsize=None)
def decoded(data):
    """jpeg_progressive.decode, once per stream"""
    return P.decode(data)


def natural_quantisers(frame):
    """[component] -> the 64 quantisers in natural order under K_ZZ_T81"""
    assert frame.standard_zigzag
    return [frame.quantiser(c.tq) for c in frame.comps]


_EXPECTED = {}


def model_expected(data, frame):
    """-> (status, coefficients in the download's layout, H x W x 3 picture, H x W luma plane); computed once per stream (the frame is
    the one the stream's own header states) and never changed."""
    assert frame.sampling() != "440", "outside the flag's envelope"
    if data in _EXPECTED:
        return _EXPECTED[data]
    d = decoded(data)
    coef = J.intent_buffer(frame, d.as_intent())
    qts = natural_quantisers(frame)
    args = (frame.width, frame.height, len(frame.comps), frame.hs, frame.vs)
    rgb = M.decode(coef, qts, *args)
    luma = M.plane_from_units(M.idct_units(M.unit_grids(coef, *args)[0], np.asarray(qts[0]).reshape(64)))
    luma = np.ascontiguousarray(luma[:frame.height, :frame.width])
    for a in (coef, rgb, luma):
        a.setflags(write=False)
    _EXPECTED[data] = (d.status, coef, rgb, luma)
    return _EXPECTED[data]


def model_coefficients(data, frame):
    """(status, coefficients in the download's layout) alone: what any sampling has, 4:4:0 included"""
    d = decoded(data)
    return d.status, J.intent_buffer(frame, d.as_intent())


# ---- the committed fixtures -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


def _read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@functools.lru_cache(maxsize=1)
def fixtures():
    """[(name, jpeg, frame, case)] in name order"""
    out = []
    for name, c in sorted(manifest()["cases"].items()):
        data = _read(name + ".jpg")
        out.append((name, data, frame_of_jpeg(data), c))
    return out


@functools.lru_cache(maxsize=None)
def record(name):
    """(Pillow's RGB decode, Pillow's draft("L") decode) as committed"""
    c = manifest()["cases"][name]
    rgb = np.frombuffer(_read(name + ".rgb"), np.uint8).reshape(c["height"], c["width"], 3)
    l8 = np.frombuffer(_read(name + ".l8"), np.uint8).reshape(c["height"], c["width"])
    return rgb, l8


def script_of(case_scans):
    """The scan script a manifest records (one compact JSON object per scan) -> [jpeg_progressive.S]"""
    tup = lambda v: tuple(tup(x) for x in v) if isinstance(v, list) else v
    return [P.S(**{k: tup(v) for k, v in json.loads(s).items()}) for s in case_scans]


def incomplete_stream(name, dropped=4):
    """The member rewritten with its last `dropped` scans missing: the same coefficients, not fully refined.  -> (jpeg, frame)"""
    _, data, frame, c = next(x for x in fixtures() if x[0] == name)
    return P.build(frame, decoded(data).coef, script_of(c["script"])[:-dropped]).data, frame


def incomplete_record(name):
    """Pillow's decode of incomplete_stream(name), as committed"""
    c = manifest()["cases"][name]
    return np.frombuffer(_read(name + ".incomplete.rgb"), np.uint8).reshape(c["height"], c["width"], 3)


# ---- the hand-built corpus ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _corpus():
    return [(label, w.data, w.frame) for label, w in PC.corpus()]


def corpus_items():
    return [x for x in _corpus() if x[2].sampling() != "440"]


def refused_items():
    return [x for x in _corpus() if x[2].sampling() == "440"]


@functools.lru_cache(maxsize=1)
def broken_items():
    return [(x[0], x[1], x[2]) for x in PC.broken()[::9] if x[2].sampling() != "440"] + PC.desynchronised()


def edge_frame(sub, w, h):
    """progressive_corpus.frame_of with odd quantisers: under the reference's arithmetic (int16)(-32768 * q) stays -32768"""
    fr = PC.frame_of(sub, w, h)
    for t in fr.qt:
        fr.qt[t] = [2 * ((k * 7 + t * 3) % 20) + 1 for k in range(64)]
    return fr


@functools.lru_cache(maxsize=1)
def edge_items():
    out = []
    for label, fr, scans in P.edge_streams(edge_frame):
        data, it = P.write(fr, scans, SC.dc_general(), SC.ac_162())
        assert (it.slots[:, 52] == -32768).any() and (it.slots[:, 0] == -32768).any(), label
        assert np.array_equal(decoded(data).coef, it.slots), label
        out.append((label, data, fr))
    return out
