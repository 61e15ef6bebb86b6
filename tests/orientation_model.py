"""A numpy model of the orientation on decode (include/pjd.h, pjd_batch_set_orientation), composed from the models that exist and
three numpy steps:

    orient(Q, o)                                = H^h(V^v(T^t(Q)))           transpose first, then the mirrors
    oriented(P, win, out_w, out_h, o, filter)   = orient(window(P, win, Q's target), o),   Q's target = out_h x out_w where t = 1

and, for the tests' own sanity, the pictures WRONG implementations would deliver (wrong_models): a case whose expectation equals one of
them would pass on a kernel with that bug, so the fixtures assert that it does not."""
import numpy as np

import resize_aa_model
import resize_bicubic_model
import resize_model
import resize_window_model as wm

FILTERS = ("bilinear", "antialias", "bicubic")
#        o:  1          2          3          4          5          6          7          8
TVH = (None, (0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))


def orient(Q, o):
    """H x W x C (or H x W) -> the picture in orientation o: exactly the three steps of include/pjd.h's table."""
    t, v, h = TVH[o]
    D = np.asarray(Q)
    if t:
        D = np.swapaxes(D, 0, 1)
    if v:
        D = D[::-1]
    if h:
        D = D[:, ::-1]
    return np.ascontiguousarray(D)


def _model(filt):
    return {"bilinear": resize_model.resize, "antialias": resize_aa_model.resize, "bicubic": resize_bicubic_model.resize}[filt]


def window(rgb, win, tw, th, filt="bilinear"):
    """flip(model(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]) of include/pjd.h with any of the three filters: th x tw x 3."""
    P = np.asarray(rgb)
    r = wm.resolve(win, P.shape[1], P.shape[0], tw, th)
    v = _model(filt)(P[r["y"]:r["y"] + r["h"], r["x"]:r["x"] + r["w"]], r["vw"], r["vh"])
    out = v[r["oy"]:r["oy"] + th, r["ox"]:r["ox"] + tw]
    return np.ascontiguousarray(out[:, ::-1] if r["flags"] & wm.HFLIP else out)


def q_target(out_w, out_h, o):
    """(tw, th) of Q for the delivered out_w x out_h."""
    return (out_h, out_w) if TVH[o][0] else (out_w, out_h)


def oriented(rgb, win, out_w, out_h, o, filt="bilinear"):
    """What a batch delivers for the picture rgb (H x W x 3 at its decode size): out_h x out_w x 3."""
    tw, th = q_target(out_w, out_h, o)
    D = orient(window(rgb, win, tw, th, filt), o)
    assert D.shape == (out_h, out_w, 3)
    return D


def _valid(win, sw, sh, tw, th):
    try:
        wm.resolve(win, sw, sh, tw, th)
        return True
    except AssertionError:
        return False


def wrong_models(rgb, win, out_w, out_h, o, filt="bilinear"):
    """{name: out_h x out_w x 3 picture} of the wrong implementations that apply to this case:
    ignored          the orientation ignored: Q to the delivered size (o != 1; where the window is valid against that target);
    no_mirrors       the transpose without the mirrors (t = 1 with v or h);
    exchanged_6_8    6 delivered as 8 and 8 as 6 (o = 6, 8);
    mirrors_first    T(H^h(V^v(Q))): the mirrors applied before the transpose (t = 1; equal to the right picture where v == h);
    unswapped_target the window resolved against the unswapped target: Q's virtual target out_w x out_h instead of out_h x out_w where
                     the window leaves it to the default (t = 1, out_w != out_h, vw or vh zero, and the window valid that way)."""
    P = np.asarray(rgb)
    sh, sw, _ = P.shape
    t, v, h = TVH[o]
    tw, th = q_target(out_w, out_h, o)
    Q = window(P, win, tw, th, filt)
    out = {}
    r = wm.resolve(win, sw, sh, tw, th)
    inside_16x = filt == "bilinear" or (r["w"] <= 16 * (r["vw"] if (win or {}).get("vw") else out_w) and r["h"] <= 16 * (r["vh"] if (win or {}).get("vh") else out_h))
    if o != 1 and _valid(win, sw, sh, out_w, out_h) and inside_16x:
        out["ignored"] = window(P, win, out_w, out_h, filt)
    if t and (v or h):
        out["no_mirrors"] = orient(Q, 5)
    if o in (6, 8):
        out["exchanged_6_8"] = orient(Q, 14 - o)
    if t and v != h:
        M = Q[::-1] if v else Q
        M = M[:, ::-1] if h else M
        out["mirrors_first"] = np.ascontiguousarray(np.swapaxes(M, 0, 1))
    w = dict(win or {})
    if t and out_w != out_h and not (w.get("vw") and w.get("vh")):
        w2 = dict(w, vw=w.get("vw") or out_w, vh=w.get("vh") or out_h)
        if _valid(w2, sw, sh, tw, th):
            out["unswapped_target"] = orient(window(P, w2, tw, th, filt), o)
    return out


def assert_not_a_wrong_model(rgb, win, out_w, out_h, o, filt, want, what):
    """A vacuous case is a test bug: the expectation must differ from every wrong model that applies.  -> the names met."""
    wrong = wrong_models(rgb, win, out_w, out_h, o, filt)
    for name, pic in wrong.items():
        assert pic.shape != want.shape or not np.array_equal(pic, want), (what, "the expectation is also that of the wrong model", name)
    return set(wrong)
