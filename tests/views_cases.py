"""What tests/test_gpu_views.py and tests/views_torch_cases.py share: five fixtures, eight views of them, and every view's expectation.

An expectation is never something this library delivered: it is tests/resize_pad_model.py (the window, filter, orientation and pad
models of the resize tests, composed) over the oracle's picture of the view's fixture, then tests/normalize_model.py for the float
types.  A grey batch is channel 0 of the same models over the oracle's plane (tests/gray_expected.py) in three equal channels."""
import os

import numpy as np

import gray_expected as G
import normalize_model as nm
import resize_pad_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61", "gray_33x70", "err_truncated_eoi_420"]
VIEWS = [2, 0, 0, 3, 2, 2, 4, 0]                             # picture 1 has no view; pictures 0 and 2 have three
FILTERS = ("bilinear", "antialias", "bicubic")
FILL = (114, 7, 201)
PAD_VALUE = (0.5, -1.0, 3e-6)
# per view: (Q's target (tw, th) -- the content, before the orientation transposes it --, orientation, pad (left, top, right, bottom) of
# the delivered canvas, window in the stored picture's coordinates or None).  Targets from 7 x 5 to 96 x 96: one and several row
# tiles, the ragged last lane group (widths 7, 19, 23, 33 are no multiple of 4), the transposed store epilogue (orientations 6 and 8),
# both mirrors, a window with a virtual target and offsets, a mirrored window, an identity view (61 x 45 of the 61 x 45 picture)
SPEC = [((7, 5), 1, (0, 0, 0, 0), None),
        ((96, 96), 6, (1, 2, 3, 0), dict(x=3, y=5, w=40, h=30, flags=1)),
        ((33, 17), 1, (0, 0, 0, 0), None),
        ((19, 11), 3, (5, 3, 6, 4), dict(x=1, y=2, w=30, h=60, vw=25, vh=14, ox=4, oy=2)),
        ((50, 64), 8, (0, 1, 0, 0), dict(x=5, y=7, w=33, h=41)),
        ((23, 29), 2, (2, 0, 0, 5), dict(flags=1)),
        ((40, 31), 4, (0, 0, 1, 1), None),
        ((61, 45), 1, (0, 0, 0, 0), None)]
assert len(SPEC) == len(VIEWS)


def golden_bytes(name):
    with open(os.path.join(HERE, "golden", name + ".jpg"), "rb") as f:
        return f.read()


def canvas(v):
    """(out_h, out_w) of view v, as set_resize takes it."""
    (tw, th), o, pad, _ = SPEC[v]
    cw, ch = (th, tw) if o >= 5 else (tw, th)
    return (ch + pad[1] + pad[3], cw + pad[0] + pad[2])


def constants():
    return (1.0 / (255.0 * np.asarray(nm.IMAGENET_STD, np.float64))).astype(np.float32), (-np.asarray(nm.IMAGENET_MEAN, np.float64) / np.asarray(nm.IMAGENET_STD, np.float64)).astype(np.float32)


_oracle = {}


def oracle(port):
    """{name: (status, rgb picture, plane)}: computed once, read-only."""
    if not _oracle:
        for n in NAMES:
            o = port.decode(golden_bytes(n))
            st, plane = G.ref_plane(port, golden_bytes(n))
            assert st == o["huff_rc"]
            rgb = np.ascontiguousarray(o["rgb"])
            rgb.setflags(write=False); plane.setflags(write=False)
            _oracle[n] = (int(st), rgb, plane)
    return _oracle


_u8 = {}


def expected_u8(port, v, filt, gray):
    """The uint8 canvas of view v, (H, W, 3): for a grey batch three equal channels."""
    key = (v, filt, gray)
    if key not in _u8:
        _, rgb, plane = oracle(port)[NAMES[VIEWS[v]]]
        src = np.repeat(plane[:, :, None], 3, axis=2) if gray else rgb
        _, o, pad, win = SPEC[v]
        h, w = canvas(v)
        fill = (FILL[0],) * 3 if gray else FILL
        C = pm.padded(src, win, w, h, pad, fill, o, filt)
        C.setflags(write=False)
        _u8[key] = C
    return _u8[key]


def expected(port, v, filt, layout, dtype=0, pad_value=None):
    """View v as download() returns it for layout "planar" (3, H, W), "rgb8" (H, W, 3) or "gray" (H, W)."""
    gray = layout == "gray"
    C = expected_u8(port, v, filt, gray)
    if dtype:
        scale, bias = constants()
        h, w = canvas(v)
        if gray:
            scale, bias = [scale[0]] * 3, [bias[0]] * 3
            pad_value = None if pad_value is None else (pad_value[0],) * 3
        C = pm.normalized(C, w, h, SPEC[v][2], dtype, scale, bias, pad_value)
    if gray:
        return np.ascontiguousarray(C[..., 0])
    return np.ascontiguousarray(C.transpose(2, 0, 1)) if layout == "planar" else np.ascontiguousarray(C)


def same(got, want, dtype, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(nm.bits(got) != nm.bits(want)) if dtype else np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing sample", bad[0].tolist(), "differing", len(bad))
