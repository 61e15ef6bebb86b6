"""A numpy model of the pad on decode (include/pjd.h, pjd_batch_set_resize_pad and pjd_batch_set_pad_value), written from the header and
composed from the models that exist and one paste:

    padded(P, win, out_w, out_h, pad, fill, o, filter)   C = fill everywhere;  C[top:top+ch, left:left+cw] = D
                                                         D = orientation_model.oriented(P, win, cw, ch, o, filter), the cw x ch picture
                                                         the batch would deliver to a target of the CONTENT's size
    normalized(C, pad, dtype, scale, bias, pad_value)    normalize_model.normalize(C), the fill included; with a pad value the border
                                                         elements are value[c] converted once to the dtype instead

pad = (left, top, right, bottom) in the DELIVERED canvas's coordinates: neither the orientation nor PJD_RW_HFLIP moves the rectangle.
And, for the tests' own sanity, the canvases WRONG implementations would deliver (wrong_models, wrong_models_float): a case whose
expectation equals one of them would pass on a kernel with that bug, so the fixtures assert that it does not."""
import numpy as np

import normalize_model as nm
import orientation_model as om
import resize_window_model as wm

WRONG = ("pad_ignored", "left_right_exchanged", "top_bottom_exchanged", "pad_permuted_by_orientation", "rectangle_mirrored_by_hflip",
         "row_stride_from_content", "fill_not_normalised", "fill_normalised_despite_pad_value")


def content(out_w, out_h, pad):
    """(cw, ch) of the content rectangle; the test of pjd_resize_pad_check as an assertion."""
    left, top, right, bottom = (int(v) for v in pad)
    assert min(left, top, right, bottom) >= 0 and left + right < out_w and top + bottom < out_h, (out_w, out_h, pad)
    return out_w - left - right, out_h - top - bottom


def paste(D, out_w, out_h, pad, fill):
    """The canvas out_h x out_w x 3 with D in its rectangle and fill[c] everywhere else."""
    cw, ch = content(out_w, out_h, pad)
    assert D.shape == (ch, cw, 3), (D.shape, cw, ch)
    C = np.empty((out_h, out_w, 3), np.uint8)
    C[:] = np.asarray(fill, np.uint8)
    C[pad[1]:pad[1] + ch, pad[0]:pad[0] + cw] = D
    return C


def padded(rgb, win, out_w, out_h, pad, fill=(0, 0, 0), o=1, filt="bilinear"):
    """What a padded batch delivers for the picture rgb (H x W x 3 at its decode size): out_h x out_w x 3 uint8."""
    cw, ch = content(out_w, out_h, pad)
    return paste(om.oriented(rgb, win, cw, ch, o, filt), out_w, out_h, pad, fill)


def border_mask(out_w, out_h, pad):
    """out_h x out_w bool: True outside the content rectangle."""
    cw, ch = content(out_w, out_h, pad)
    m = np.ones((out_h, out_w), bool)
    m[pad[1]:pad[1] + ch, pad[0]:pad[0] + cw] = False
    return m


def convert(value, dtype):
    """One binary32 value converted once to the dtype, to nearest even: an element of nm.NP_TYPE[dtype] (bfloat16 as its bits)."""
    u = np.float32(value)
    if dtype == nm.DT_F32:
        return u
    if dtype == nm.DT_F16:
        with np.errstate(over="ignore"):
            return u.astype(np.float16)
    return nm.to_bf16_bits(u).reshape(())[()]


def normalized(C, out_w, out_h, pad, dtype, scale, bias, pad_value=None):
    """The canvas C (uint8, fill included) as the normalised batch delivers it: out_h x out_w x 3 in nm.NP_TYPE[dtype]."""
    out = nm.normalize(C, dtype, scale, bias)
    if pad_value is not None:
        m = border_mask(out_w, out_h, pad)
        for c in range(3):
            out[..., c][m] = convert(pad_value[c], dtype)
    return out


# ---- what wrong implementations would deliver ------------------------------------------------------------------------------------------
def _try(f):
    try:
        return f()
    except AssertionError:
        return None


def wrong_models(rgb, win, out_w, out_h, pad, fill, o=1, filt="bilinear"):
    """{name: out_h x out_w x 3 canvas} of the wrong implementations that apply to this case:
    pad_ignored                  the content stretched over the whole canvas (a pad that is not all zero; where the window is valid so);
    left_right_exchanged         the record read as (right, top, left, bottom) (left != right);
    top_bottom_exchanged         ... as (left, bottom, right, top) (top != bottom);
    pad_permuted_by_orientation  the pad applied in Q's frame and the whole canvas oriented: the rectangle moves with the orientation
                                 (o != 1 and a record the orientation does not map onto itself; where Q's canvas less the record still
                                 holds a sample and the window is valid so);
    rectangle_mirrored_by_hflip  PJD_RW_HFLIP mirroring the rectangle with its content (a window with the flag, left != right);
    row_stride_from_content      the content's rows stored cw samples apart from the rectangle's first sample, not out_w -- for a
                                 transposed picture store_cols with the content's row length -- and the border filled behind it
                                 (ch > 1 and cw != out_w)."""
    left, top, right, bottom = pad
    cw, ch = content(out_w, out_h, pad)
    D = om.oriented(rgb, win, cw, ch, o, filt)
    out = {}
    if any(pad):
        p = _try(lambda: om.oriented(rgb, win, out_w, out_h, o, filt))
        if p is not None:
            out["pad_ignored"] = p
    if left != right:
        out["left_right_exchanged"] = paste(D, out_w, out_h, (right, top, left, bottom), fill)
    if top != bottom:
        out["top_bottom_exchanged"] = paste(D, out_w, out_h, (left, bottom, right, top), fill)
    if o != 1:
        qw, qh = om.q_target(out_w, out_h, o)

        def permuted():
            qcw, qch = content(qw, qh, pad)
            return om.orient(paste(om.window(rgb, win, qcw, qch, filt), qw, qh, pad, fill), o)
        # not where the orientation maps the rectangle onto itself (a record with that symmetry): that canvas is the right one
        moved = _try(lambda: not np.array_equal(om.orient(border_mask(qw, qh, pad), o), border_mask(out_w, out_h, pad)))
        p = _try(permuted) if moved else None
        if p is not None:
            out["pad_permuted_by_orientation"] = p
    if (win or {}).get("flags", 0) & wm.HFLIP and left != right:
        out["rectangle_mirrored_by_hflip"] = paste(D, out_w, out_h, (right, top, left, bottom), fill)
    if ch > 1 and cw != out_w:
        flat = np.empty((out_h * out_w, 3), np.uint8)
        flat[:] = np.asarray(fill, np.uint8)
        first = top * out_w + left
        flat[first:first + ch * cw] = D.reshape(ch * cw, 3)
        C = flat.reshape(out_h, out_w, 3)
        C[border_mask(out_w, out_h, pad)] = np.asarray(fill, np.uint8)
        out["row_stride_from_content"] = C
    return out


def wrong_models_float(C, out_w, out_h, pad, fill, dtype, scale, bias, pad_value=None):
    """{name: normalised canvas} for the canvas C of a normalised batch:
    fill_not_normalised               the border holds fill[c] itself, converted to the dtype (a pad that is not all zero, no pad value);
    fill_normalised_despite_pad_value the border holds the normalised fill although a pad value is set."""
    out = {}
    if not any(pad):
        return out
    if pad_value is None:
        out["fill_not_normalised"] = normalized(C, out_w, out_h, pad, dtype, scale, bias, pad_value=[float(v) for v in fill])
    else:
        out["fill_normalised_despite_pad_value"] = normalized(C, out_w, out_h, pad, dtype, scale, bias)
    return out


def assert_not_a_wrong_model(wrong, want, what, bits=False):
    """A vacuous case is a test bug: the expectation must differ from every wrong model that applies.  -> the names met."""
    for name, pic in wrong.items():
        same = pic.shape == want.shape and (np.array_equal(nm.bits(pic), nm.bits(want)) if bits else np.array_equal(pic, want))
        assert not same, (what, "the expectation is also that of the wrong model", name)
    return set(wrong)
