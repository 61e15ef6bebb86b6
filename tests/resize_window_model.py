"""A numpy model of the windowed resize (include/pjd.h, pjd_batch_set_resize_window), composed from the two models that exist --
resize_model.resize and resize_aa_model.resize -- and nothing else: crop -> model -> crop -> flip.

    window(P, win, tw, th, antialias) = flip(model(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw])

and, for the tests' own sanity, the pictures four WRONG implementations would deliver (wrong_models): a case whose expectation
equals one of them would pass on a kernel with that bug, so the fixtures assert that it does not."""
import numpy as np

import resize_aa_model as aa
import resize_model

HFLIP = 1
FIELDS = ("x", "y", "w", "h", "vw", "vh", "ox", "oy", "flags")


def resolve(win, sw, sh, tw, th):
    """The nine fields of a window (a dict, None: all zero) with the defaults of include/pjd.h resolved, as a dict."""
    r = {k: int((win or {}).get(k, 0)) for k in FIELDS}
    assert set(win or {}) <= set(FIELDS)
    if r["w"] == 0 and r["h"] == 0:
        assert r["x"] == 0 and r["y"] == 0
        r["w"], r["h"] = sw, sh
    r["vw"], r["vh"] = r["vw"] or tw, r["vh"] or th
    assert 1 <= r["w"] and r["x"] + r["w"] <= sw and 1 <= r["h"] and r["y"] + r["h"] <= sh
    assert r["ox"] + tw <= r["vw"] and r["oy"] + th <= r["vh"]
    return r


def _model(antialias):
    return aa.resize if antialias else resize_model.resize


def window(rgb, win, tw, th, antialias=False):
    """H x W x 3 uint8 (the picture at its decode size) -> th x tw x 3 uint8."""
    P = np.asarray(rgb)
    r = resolve(win, P.shape[1], P.shape[0], tw, th)
    v = _model(antialias)(P[r["y"]:r["y"] + r["h"], r["x"]:r["x"] + r["w"]], r["vw"], r["vh"])
    out = v[r["oy"]:r["oy"] + th, r["ox"]:r["ox"] + tw]
    return np.ascontiguousarray(out[:, ::-1] if r["flags"] & HFLIP else out)


# ---- what wrong implementations would deliver ------------------------------------------------------------------------------------------
def _bilinear_taps_picture_clamp(sn, x, w, vw):
    """The bilinear taps of a window [x, x + w) of an axis of sn samples over vw target samples, with the sample position clamped to
    the PICTURE: absolute (i0, i1, weight)."""
    i = np.arange(vw, dtype=np.int64)
    X = np.clip((2 * i + 1) * w - vw + 2 * vw * x, 0, 2 * vw * (sn - 1))
    i0 = X // (2 * vw)
    return i0, np.minimum(i0 + 1, sn - 1), ((X - i0 * 2 * vw) * 256 + vw) // (2 * vw)


def _aa_matrix_picture_clamp(sn, x, w, vw):
    """The antialiased weights (vw x sn, in 1/65536) of that window where the samples dropped are those outside the PICTURE."""
    S = max(w, vw)
    j = np.arange(sn, dtype=np.int64)
    M = np.zeros((vw, sn), dtype=np.int64)
    for i in range(vw):
        r = np.maximum(0, 2 * S - np.abs((2 * (j - x) + 1) * vw - (2 * i + 1) * w))
        R = int(r.sum())
        q = (r * 65536 + R // 2) // R
        q[int(r.argmax())] += 65536 - int(q.sum())
        M[i] = q
    return M


def _reaches_outside(sn, x, w, vw, o, t, antialias):
    """Whether the picture-clamped taps of the delivered samples [o, o + t) of an axis give weight to a sample outside [x, x + w)."""
    inside = np.zeros(sn, bool)
    inside[x:x + w] = True
    if antialias:
        return bool(_aa_matrix_picture_clamp(sn, x, w, vw)[o:o + t][:, ~inside].any())
    i0, i1, wt = (a[o:o + t] for a in _bilinear_taps_picture_clamp(sn, x, w, vw))
    return bool((~inside[i0] & (wt < 256)).any() or (~inside[i1] & (wt > 0)).any())


def _picture_clamp(P, r, antialias):
    P = P.astype(np.int64)
    sh, sw, _ = P.shape
    if antialias:
        Mx, My = _aa_matrix_picture_clamp(sw, r["x"], r["w"], r["vw"]), _aa_matrix_picture_clamp(sh, r["y"], r["h"], r["vh"])
        h16 = (np.einsum("ij,yjc->yic", Mx, P) + 128) >> 8
        return ((np.einsum("iy,yxc->ixc", My, h16) + (1 << 23)) >> 24).astype(np.uint8)
    x0, x1, wx = _bilinear_taps_picture_clamp(sw, r["x"], r["w"], r["vw"])
    y0, y1, wy = _bilinear_taps_picture_clamp(sh, r["y"], r["h"], r["vh"])
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = (256 - wx) * P[y0][:, x0] + wx * P[y0][:, x1]
    bot = (256 - wx) * P[y1][:, x0] + wx * P[y1][:, x1]
    return (((256 - wy) * top + wy * bot + 32768) >> 16).astype(np.uint8)


def wrong_models(rgb, win, tw, th, antialias=False):
    """{name: th x tw x 3 picture} of the wrong implementations that apply to this case:
    no_window      the record ignored: the whole picture resized to tw x th (any non-zero record);
    picture_clamp  the right taps, but samples outside the window taken from the picture where it has pixels there, and clamped /
                   dropped only at the picture's edge (a window that is not the whole picture, on an axis where the filter reaches
                   past the window for a delivered sample);
    no_flip        the mirror ignored (PJD_RW_HFLIP set, more than one column);
    no_offset      ox and oy ignored: the top-left tw x th of the virtual target (a non-zero offset on an axis with more than one sample)."""
    P = np.asarray(rgb)
    sh, sw, _ = P.shape
    r = resolve(win, sw, sh, tw, th)
    flip = lambda a: np.ascontiguousarray(a[:, ::-1] if r["flags"] & HFLIP else a)
    out = {}
    if any((win or {}).get(k, 0) for k in FIELDS):
        out["no_window"] = _model(antialias)(P, tw, th)
    # picture_clamp applies where, for a DELIVERED sample, that implementation's taps touch the picture outside the window (decided on
    # the taps alone, not on what the pictures hold): never for bilinear on a shrinking axis (the outermost sample position,
    # (w/vw - 1)/2 from the edge, is inside), never where the delivered part stays clear of the virtual target's edges
    if _reaches_outside(sw, r["x"], r["w"], r["vw"], r["ox"], tw, antialias) or _reaches_outside(sh, r["y"], r["h"], r["vh"], r["oy"], th, antialias):
        out["picture_clamp"] = flip(_picture_clamp(P, r, antialias)[r["oy"]:r["oy"] + th, r["ox"]:r["ox"] + tw])
    # a window of one column gives identical columns (mirror and column offset change nothing), one of one row identical rows
    if r["flags"] & HFLIP and r["w"] > 1 and tw > 1:
        out["no_flip"] = window(P, dict(r, flags=0), tw, th, antialias)
    if (r["ox"] and r["w"] > 1) or (r["oy"] and r["h"] > 1):
        out["no_offset"] = window(P, dict(r, ox=0, oy=0), tw, th, antialias)
    return out
