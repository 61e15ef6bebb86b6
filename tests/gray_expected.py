"""Expected planes of PJD_OUT_GRAY8 (include/pjd.h, "grey output"), shared by tests/test_gray_cpu.py and tests/test_gpu_gray.py.  Never
from the code under test:

* reference arithmetic: the oracle port's coefficients with components 1 and 2 zeroed, through its own DPU stages and raster -- the
  picture P0 of the definition, whose three channels are equal; the expected plane is channel 0;
* libjpeg: tests/golden/libjpeg_gray/<name>.l8, Pillow's draft("L") decode of the files of tests/golden/libjpeg/.
"""
import functools
import json
import os

import numpy as np

import libjpeg_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_GRAY = os.path.join(HERE, "golden", "libjpeg_gray")
GOLD_LJ = os.path.join(HERE, "golden", "libjpeg")


def golden_bytes(name):
    with open(os.path.join(HERE, "golden", name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=1)
def lj_cases():
    """The cases of tests/golden/libjpeg/manifest.json: name -> width, height, sampling, progressive, restart_marker_blocks, ..."""
    with open(os.path.join(GOLD_LJ, "manifest.json")) as f:
        return json.load(f)["cases"]


def lj_bytes(name):
    with open(os.path.join(GOLD_LJ, name + ".jpg"), "rb") as f:
        return f.read()


def lj_rgb(name):
    """Pillow's recorded colour decode of a libjpeg fixture (H x W x 3)."""
    c = lj_cases()[name]
    with open(os.path.join(GOLD_LJ, name + ".rgb"), "rb") as f:
        return np.frombuffer(f.read(), np.uint8).reshape(c["height"], c["width"], 3)


def lj_baseline_cases():
    return sorted(n for n, c in lj_cases().items() if not c["progressive"] and not c["restart_marker_blocks"])


def neutral_chroma_picture(port, data):
    """(status, H x W x 3 picture) of the oracle with every chroma coefficient zero.  The coefficient layout of a DPU payload is
    blk16 * 768 + comp * 256 + pos * 64 + k; behind an entropy-coding error the oracle's coefficients are zero already."""
    o = port.decode(data)
    assert o["valid"]
    info, meta = o["info"], o["metadata"]
    mcus = o["coef"].copy()
    n_dpus = mcus.shape[0]
    mcus.reshape(n_dpus, 25, 3, 256)[:, :, 1:, :] = 0
    for d in range(n_dpus):
        port.L.orc_dpu_exec(meta.ctypes.data, mcus[d].ctypes.data)
    rgb = np.zeros((info["height"], info["width"], 3), np.uint8)
    port.L.orc_rgb_from_mcus(meta.ctypes.data, mcus.ctypes.data, rgb.ctypes.data)
    return o["huff_rc"], rgb


def ref_plane_of_coefficients(port, twin, coef):
    """The expected H x W plane under the reference's arithmetic for coefficients given in the download's layout (n_dpus x 19200), as
    neutral_chroma_picture makes it: a progressive frame, which the oracle cannot entropy-decode, brings the coefficients of the
    model of tests/jpeg_progressive.py and `twin`, a baseline file of the same frame, for the metadata.  The caller sets the port's
    zigzag map."""
    o = port.parse(twin)
    assert o["info"]["valid"]
    meta = o["metadata"]
    mcus = np.array(coef, np.int16).reshape(-1, 19200)
    mcus.reshape(mcus.shape[0], 25, 3, 256)[:, :, 1:, :] = 0
    for d in range(mcus.shape[0]):
        port.L.orc_dpu_exec(meta.ctypes.data, mcus[d].ctypes.data)
    rgb = np.zeros((o["info"]["height"], o["info"]["width"], 3), np.uint8)
    port.L.orc_rgb_from_mcus(meta.ctypes.data, mcus.ctypes.data, rgb.ctypes.data)
    assert np.array_equal(rgb[:, :, 0], rgb[:, :, 1]) and np.array_equal(rgb[:, :, 0], rgb[:, :, 2])
    return np.ascontiguousarray(rgb[:, :, 0])


def ref_plane(port, data):
    """(status, expected H x W plane) under the reference's arithmetic."""
    st, rgb = neutral_chroma_picture(port, data)
    return st, np.ascontiguousarray(rgb[:, :, 0])


@functools.lru_cache(maxsize=1)
def gray_manifest():
    with open(os.path.join(GOLD_GRAY, "manifest.json")) as f:
        return json.load(f)


def l8(name):
    """The recorded plane of a libjpeg fixture."""
    c = gray_manifest()["cases"][name]
    with open(os.path.join(GOLD_GRAY, name + ".l8"), "rb") as f:
        return np.frombuffer(f.read(), np.uint8).reshape(c["height"], c["width"])


def model_y_plane(port, data, broken=False):
    """The Y plane of tests/libjpeg_model.py over the oracle port's coefficients (T.81 zigzag) of a baseline file.  broken: the stream
    has an entropy-coding error -- the port's coefficients are zero behind it -- and the result is (status, plane)."""
    port.standard_zigzag(True)
    try:
        d = port.decode(data)
    finally:
        port.standard_zigzag(False)
    info = d["info"]
    assert broken or d["huff_rc"] == 0
    grids = M.unit_grids(d["coef"], info["width"], info["height"], info["ncomp"], info["hsamp"], info["vsamp"])
    q = np.asarray(info["qt"][info["comp_qt"][0]]).reshape(64)
    plane = M.plane_from_units(M.idct_units(grids[0], q))[:info["height"], :info["width"]]
    return (d["huff_rc"], plane) if broken else plane


def truncated_lj():
    """lj_33x31_420_q100 (3 x 2 MCUs, dense) with its entropy-coded data cut to a fifth: the error lies in the first MCU row."""
    data = lj_bytes("lj_33x31_420_q100")
    body = data.rfind(b"\xff\xda") + 14
    return data[:body + (len(data) - 2 - body) // 5] + b"\xff\xd9"


def misplaced_restart_markers(port):
    """Restart-segmented fixtures with one byte inserted before, or the byte removed before, a restart marker: a segment that ends late
    or early without an entropy-coding error of its own, which the parallel decoder flags and the exact kernel decodes again."""
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
    return [j for j in out if port.parse(j)["info"]["valid"]]


def box1(plane, s):
    """The box filter of include/pjd.h (PJD_F_SCALE_*) on one plane, written from the header: ceil(H/s) x ceil(W/s), output (i, j) =
    (sum + (n >> 1)) // n over the n source pixels of its box, boxes cut at the right and bottom edge."""
    if s == 1:
        return plane
    h, w = plane.shape
    sh, sw = -(-h // s), -(-w // s)
    acc = np.zeros((sh * s, sw * s), np.int64)
    cnt = np.zeros((sh * s, sw * s), np.int64)
    acc[:h, :w] = plane
    cnt[:h, :w] = 1
    tot, n = acc.reshape(sh, s, sw, s).sum(axis=(1, 3)), cnt.reshape(sh, s, sw, s).sum(axis=(1, 3))
    return ((tot + (n >> 1)) // n).astype(np.uint8)
