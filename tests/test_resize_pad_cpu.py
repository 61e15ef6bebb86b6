"""Pad on decode (pjd_batch_set_resize_pad), the parts that need no device: the exports, pjd_resize_pad_check on its boundaries,
tensors.letterbox_plan against exact rational arithmetic, the argument checks of the tensor helpers (which run before a context is
touched), and the numpy model (tests/resize_pad_model.py) against itself."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import normalize_model as nm
import orientation_model as om
import resize_pad_model as pm

E_ARG = -3


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_exports_exist_and_the_version_stays_6():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert L.pjd_batch_set_resize_pad and L.pjd_batch_set_pad_value and L.pjd_resize_pad_check
    fill = (C.c_uint8 * 3)(0, 0, 0)
    assert L.pjd_batch_set_resize_pad(None, (pjd_amd.ResizePad * 1)(), fill) == E_ARG     # no batch
    assert L.pjd_batch_set_pad_value(None, (C.c_float * 3)(0, 0, 0)) == E_ARG
    assert C.sizeof(pjd_amd.ResizePad) == 16 and [k for k, _ in pjd_amd.ResizePad._fields_] == ["left", "top", "right", "bottom"]
    assert hasattr(pjd_amd.Batch, "set_resize_pad") and hasattr(pjd_amd.Batch, "set_pad_value")
    assert callable(pjd_amd.resize_pad_check) and callable(pjd_amd.resize_pad)


def test_pad_check_on_its_boundaries():
    import pjd_amd
    ok = pjd_amd.resize_pad_check
    assert ok(9, 9, (0, 0, 0, 0)) and ok(1, 1, (0, 0, 0, 0))
    # a content of exactly one column, and of exactly one row, wherever it lies
    for l in range(9):
        assert ok(9, 5, (l, 0, 8 - l, 0)) and ok(5, 9, (0, l, 0, 8 - l))
    assert ok(65535, 65535, (65534, 0, 0, 65534)) and ok(65535, 65535, (0, 65534, 65534, 0))
    # left + right == out_w, top + bottom == out_h, and beyond
    for l in range(10):
        assert not ok(9, 5, (l, 0, 9 - l, 0)) and not ok(5, 9, (0, l, 0, 9 - l))
    assert not ok(9, 9, (9, 0, 0, 0)) and not ok(9, 9, (0, 0, 0, 10)) and not ok(9, 9, (5, 0, 5, 0))
    # sums that wrap 32 bits: 2^32 - 1 + 2 == 1, 2^31 + 2^31 == 0
    M = 2 ** 32 - 1
    for a, b in ((M, 2), (2, M), (2 ** 31, 2 ** 31), (M, M), (M, 1)):
        assert not ok(9, 9, (a, 0, b, 0)) and not ok(9, 9, (0, a, 0, b)), (a, b)
    # the canvas itself: 1..65535
    assert not ok(0, 9, (0, 0, 0, 0)) and not ok(9, 0, (0, 0, 0, 0)) and not ok(65536, 9, (0, 0, 0, 0)) and not ok(9, 65536, (0, 0, 0, 0))
    # a null record
    assert pjd_amd.dev_lib().pjd_resize_pad_check(9, 9, None) == E_ARG and not ok(9, 9, None)
    rec = pjd_amd.ResizePad(1, 2, 3, 4)
    assert pjd_amd.dev_lib().pjd_resize_pad_check(9, 9, C.byref(rec)) == 0
    # the model's assertion is the same test
    for W, H, pad in ((9, 9, (4, 4, 4, 4)), (9, 9, (4, 4, 5, 4)), (9, 9, (0, 8, 0, 0)), (9, 9, (0, 8, 0, 1))):
        assert ok(W, H, pad) == (pm._try(lambda: pm.content(W, H, pad)) is not None)


def test_resize_pad_records():
    import pjd_amd
    r = pjd_amd.resize_pad(dict(left=1, bottom=4))
    assert (r.left, r.top, r.right, r.bottom) == (1, 0, 0, 4)
    r = pjd_amd.resize_pad((1, 2, 3, 4))
    assert (r.left, r.top, r.right, r.bottom) == (1, 2, 3, 4)
    r2 = pjd_amd.resize_pad(r)
    assert r2 is not r and bytes(r2) == bytes(r)
    for bad in (dict(lft=1), (1, 2, 3), (1, 2, 3, 4, 5), (-1, 0, 0, 0), (2 ** 32, 0, 0, 0)):
        with pytest.raises(ValueError):
            pjd_amd.resize_pad(bad)


# ---- letterbox_plan ------------------------------------------------------------------------------------------------------------------------
def _round_half_up(x):
    return int((x + Fraction(1, 2)).__floor__())


def test_letterbox_plan_on_a_grid_against_exact_rational_arithmetic():
    from pjd_amd import tensors
    sizes = [1, 2, 3, 5, 7, 8, 13, 64, 100, 223, 224, 225, 640]
    n = 0
    for h in sizes:
        for w in sizes:
            for H, W in ((224, 224), (7, 13), (13, 7), (1, 1), (1, 9), (640, 384), (333, 500)):
                s = min(Fraction(H, h), Fraction(W, w))
                if Fraction(w, h) <= Fraction(W, H):
                    ch, cw = H, max(1, min(W, _round_half_up(w * s)))
                else:
                    cw, ch = W, max(1, min(H, _round_half_up(h * s)))
                for mode in ("center", "topleft"):
                    got = tensors.letterbox_plan((h, w), (H, W), mode)
                    assert all(isinstance(v, int) for v in got)
                    gch, gcw, l, t, r, b = got
                    assert (gch, gcw) == (ch, cw), (h, w, H, W)
                    assert l + gcw + r == W and t + gch + b == H and min(l, t, r, b) >= 0
                    if mode == "topleft":
                        assert (l, t) == (0, 0)
                    else:
                        assert r - l in (0, 1) and b - t in (0, 1)                  # centred: the odd one goes right and below
                    assert gch == H or gcw == W                                     # one side fills the canvas
                    # the aspect ratio is kept to within half a sample of the free side (unless clamped to 1)
                    if gcw > 1 and gch > 1:
                        assert abs(Fraction(gcw) - w * s) <= Fraction(1, 2) and abs(Fraction(gch) - h * s) <= Fraction(1, 2)
                    n += 1
    assert n == len(sizes) ** 2 * 7 * 2


def test_letterbox_plan_extremes_and_errors():
    from pjd_amd import tensors
    import pjd_amd
    assert tensors.letterbox_plan((1, 65535), (224, 224)) == (1, 224, 0, 111, 0, 112)          # 224 / 65535 of a row: clamped to 1
    assert tensors.letterbox_plan((65535, 1), (224, 224)) == (224, 1, 111, 0, 112, 0)
    assert tensors.letterbox_plan((65535, 1), (224, 224), "topleft") == (224, 1, 0, 0, 223, 0)
    assert tensors.letterbox_plan((300, 300), (224, 224)) == (224, 224, 0, 0, 0, 0)              # equal aspect
    assert tensors.letterbox_plan((480, 640), (240, 320)) == (240, 320, 0, 0, 0, 0)
    assert tensors.letterbox_plan((224, 224), (224, 224)) == (224, 224, 0, 0, 0, 0)              # already the canvas
    assert tensors.letterbox_plan((480, 640), (640, 640)) == (480, 640, 0, 80, 0, 80)            # YOLO's 640 letterbox of a VGA frame
    assert tensors.letterbox_plan((480, 640), (1024, 1024), "topleft") == (768, 1024, 0, 0, 0, 256)   # SAM
    assert tensors.letterbox_plan((3, 2), (5, 5)) == (5, 3, 1, 0, 1, 0)                          # 10 / 3 = 3.33 -> 3
    assert tensors.letterbox_plan((2, 1), (5, 5)) == (5, 3, 1, 0, 1, 0)                          # 2.5 -> 3: half up
    for h, w, H, W in ((1, 65535, 224, 224), (65535, 1, 224, 224), (7, 9, 1, 1), (1, 1, 65535, 65535)):
        ch, cw, l, t, r, b = tensors.letterbox_plan((h, w), (H, W))
        assert pjd_amd.resize_pad_check(W, H, (l, t, r, b)) and (cw, ch) == pm.content(W, H, (l, t, r, b))
    for bad in (((0, 5), (4, 4), "center"), ((5, 5), (0, 4), "center"), ((5, 5), (4, 4), "bottomright"), ((5, 5), (4, 4), None)):
        with pytest.raises(ValueError):
            tensors.letterbox_plan(*bad)


# ---- the argument checks of the tensor helpers: before a context is touched ------------------------------------------------------------------
def _desc(w, h):
    import pjd_amd
    d = pjd_amd.ImageDesc()
    d.width, d.height = w, h
    return d


def test_tensor_helper_argument_checks_run_before_a_context_is_touched():
    from pjd_amd import tensors
    descs = [_desc(13, 9)]
    mean, std = nm.IMAGENET_MEAN, nm.IMAGENET_STD
    for kw in (dict(letterbox="middle"), dict(letterbox="center", resize_short=8), dict(letterbox="center", fill=(0, 0)),
               dict(letterbox="center", fill=(0, 0, 256)), dict(letterbox="center", fill=(0, 0, 1.5)), dict(fill=(0, -1, 0)),
               dict(letterbox="topleft", crops=[(0, 0, 14, 9)]), dict(letterbox="center", flips=[True, False]),
               dict(letterbox="center", orientations=[9])):
        with pytest.raises(ValueError):
            tensors.decode_resized_batch_tensor(None, descs, (8, 8), prescale=False, **kw)
        with pytest.raises(ValueError):
            tensors.decode_normalized_batch_tensor(None, descs, (8, 8), mean, std, prescale=False, **kw)
    for kw in (dict(pad_value=0.0), dict(letterbox="center", pad_value=float("nan")), dict(letterbox="center", pad_value=(0, 0)),
               dict(letterbox="center", pad_value=(0, float("inf"), 0))):
        with pytest.raises(ValueError):
            tensors.decode_normalized_batch_tensor(None, descs, (8, 8), mean, std, prescale=False, **kw)


def test_the_letterbox_plan_of_the_tensor_helpers():
    """tensors._plan_letterbox, emulated with the model: the plan is made from the UPRIGHT picture (or its crop), crops and orientations
    act on the content, a flip mirrors the content inside its rectangle, and the pre-scale is picked from the content size."""
    from pjd_amd import tensors
    import pjd_amd
    rng = np.random.default_rng(5)
    P = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)                                # the stored picture: 13 x 9
    H, W = 12, 12
    for o in range(1, 9):
        U = om.orient(P, o)
        UH, UW = U.shape[:2]
        for flip in (False, True):
            run, wins, oris, pads = tensors._plan_outputs([_desc(13, 9)], (H, W), False, None, [flip], [o], None, "center")
            ch, cw, l, t, r, b = tensors.letterbox_plan((UH, UW), (H, W))
            assert pads == [(l, t, r, b)] and (cw, ch) == pm.content(W, H, pads[0])
            got = pm.padded(P, (wins or [None])[0], W, H, pads[0], (1, 2, 3), oris[0])
            D = om.oriented(P, None, cw, ch, o)
            assert np.array_equal(got, pm.paste(D[:, ::-1] if flip else D, W, H, pads[0], (1, 2, 3))), (o, flip)
        # a crop of the upright picture: the plan is the crop's, and at the crop's own size the content is the crop itself
        x, y, w, h = 1, 2, UW - 3, UH - 4
        run, wins, oris, pads = tensors._plan_outputs([_desc(13, 9)], (h + 3, w), False, [(x, y, w, h)], None, [o], None, "topleft")
        assert pads == [(0, 0, 0, 3)]                                                   # the width limits, the scale is 1
        got = pm.padded(P, wins[0], w, h + 3, pads[0], (9, 9, 9), oris[0])
        assert np.array_equal(got, pm.paste(U[y:y + h, x:x + w], w, h + 3, pads[0], (9, 9, 9))), o
    # no orientations: none are set; a flip is the window's flag
    run, wins, oris, pads = tensors._plan_outputs([_desc(13, 9), _desc(9, 13)], (12, 12), False, None, [True, False], None, None, "center")
    assert oris is None and wins == [dict(flags=pjd_amd.RW_HFLIP), None] and pads == [(0, 2, 0, 2), (2, 0, 2, 0)]
    # the pre-scale comes from the content size: 640 x 480 into 64 x 64 has a content of 64 x 48, so 1/8 (80 x 60) still covers it
    run, _, _, pads = tensors._plan_outputs([_desc(640, 480)], (64, 64), True, None, None, None, None, "center")
    assert pads == [(0, 8, 0, 8)] and int(run[0].flags) & pjd_amd.F_SCALE_MASK == tensors.pick_scale_flags(640, 480, 64, 48) == 3 << 4


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def test_zero_pads_equal_the_unpadded_model():
    rng = np.random.default_rng(3)
    P = rng.integers(0, 256, (45, 61, 3), dtype=np.uint8)
    for o in range(1, 9):
        for filt in om.FILTERS:
            for win in (None, dict(x=3, y=5, w=40, h=30, flags=1)):
                out_h, out_w = (11, 19) if o < 5 else (19, 11)
                C = pm.padded(P, win, out_w, out_h, (0, 0, 0, 0), (7, 8, 9), o, filt)
                assert np.array_equal(C, om.oriented(P, win, out_w, out_h, o, filt))
                assert not pm.wrong_models(P, win, out_w, out_h, (0, 0, 0, 0), (7, 8, 9), o, filt), "nothing can go wrong without a pad"
    assert not pm.border_mask(19, 11, (0, 0, 0, 0)).any()


def test_the_model_pastes_and_fills():
    rng = np.random.default_rng(4)
    P = rng.integers(0, 256, (45, 61, 3), dtype=np.uint8)
    pad, fill = (5, 3, 6, 4), (114, 7, 201)
    C = pm.padded(P, None, 30, 20, pad, fill, 6, "bicubic")
    m = pm.border_mask(30, 20, pad)
    assert m.sum() == 30 * 20 - 19 * 13 and (C[m] == np.asarray(fill, np.uint8)).all()
    assert np.array_equal(C[3:16, 5:24], om.oriented(P, None, 19, 13, 6, "bicubic"))
    met = pm.assert_not_a_wrong_model(pm.wrong_models(P, None, 30, 20, pad, fill, 6, "bicubic"), C, "cpu")
    assert met == {"pad_ignored", "left_right_exchanged", "top_bottom_exchanged", "pad_permuted_by_orientation", "row_stride_from_content"}
    scale, bias = np.asarray([1 / 255.0] * 3, np.float32), np.asarray([-0.5, 0.25, 0.0], np.float32)
    for dtype in (nm.DT_F16, nm.DT_BF16, nm.DT_F32):
        N = pm.normalized(C, 30, 20, pad, dtype, scale, bias)
        assert np.array_equal(nm.bits(N), nm.bits(nm.normalize(C, dtype, scale, bias)))
        for value in ((0.0, 0.0, 0.0), (3e-6, -3e-6, 1.0)):          # 3e-6 is subnormal in binary16 (below 2^-14), not zero (above 2^-25)
            V = pm.normalized(C, 30, 20, pad, dtype, scale, bias, value)
            assert np.array_equal(nm.bits(V)[~m], nm.bits(N)[~m])
            for c in range(3):
                assert (nm.bits(V[..., c])[m] == nm.bits(pm.convert(value[c], dtype))).all()
            assert pm.assert_not_a_wrong_model(pm.wrong_models_float(C, 30, 20, pad, fill, dtype, scale, bias, value), V, "cpu", bits=True) == {"fill_normalised_despite_pad_value"}
        assert pm.assert_not_a_wrong_model(pm.wrong_models_float(C, 30, 20, pad, fill, dtype, scale, bias), N, "cpu", bits=True) == {"fill_not_normalised"}
    h = pm.convert(3e-6, nm.DT_F16)
    assert 0 < int(nm.bits(h)) < 0x0400, "a binary16 subnormal"
    assert set(pm.WRONG) == {"pad_ignored", "left_right_exchanged", "top_bottom_exchanged", "pad_permuted_by_orientation", "rectangle_mirrored_by_hflip",
                             "row_stride_from_content", "fill_not_normalised", "fill_normalised_despite_pad_value"}
