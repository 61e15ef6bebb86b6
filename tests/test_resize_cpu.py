"""Resize on decode, the parts that need no GPU: the exports, the tap computation (pjd_resize_tap: the code the kernel runs) against
the numpy model of include/pjd.h's text, the model against float64 bilinear, pick_scale_flags, the descriptor copies."""
import ctypes as C

import numpy as np
import pytest

import resize_model

SIZES = [1, 2, 3, 7, 8, 61, 224, 256, 500, 640, 4000, 65535]
E_ARG = -3


def test_exports_and_abi_version():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_batch_set_resize") and hasattr(L, "pjd_resize_tap")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION


def _lib_taps(sn, dn):
    import pjd_amd
    L = pjd_amd.dev_lib()
    a, b, w = C.c_uint32(), C.c_uint32(), C.c_uint32()
    out = np.zeros((3, dn), np.int64)
    for i in range(dn):
        assert L.pjd_resize_tap(sn, dn, i, C.byref(a), C.byref(b), C.byref(w)) == 0
        out[0, i], out[1, i], out[2, i] = a.value, b.value, w.value
    return out


def _pairs():
    pairs = [(s, d) for s in SIZES for d in SIZES]
    rng = np.random.default_rng(20)
    for _ in range(200):
        hi = int(rng.choice([16, 300, 5000, 65535]))
        pairs.append((int(rng.integers(1, hi + 1)), int(rng.integers(1, hi + 1))))
    return pairs


def test_tap_export_equals_the_model_for_every_index():
    for sn, dn in _pairs():
        got = _lib_taps(sn, dn)
        i0, i1, w = resize_model.taps(sn, dn)
        assert np.array_equal(got[0], i0) and np.array_equal(got[1], i1) and np.array_equal(got[2], w), (sn, dn)
        assert w.min() >= 0 and w.max() <= 256 and i1.max() <= sn - 1


def test_tap_error_returns():
    import pjd_amd
    L = pjd_amd.dev_lib()
    a = C.c_uint32()
    for sn, dn, i in [(0, 5, 0), (5, 0, 0), (65536, 5, 0), (5, 65536, 0), (5, 5, 5), (5, 5, 2 ** 32 - 1), (65535, 65535, 65535)]:
        assert L.pjd_resize_tap(sn, dn, i, C.byref(a), C.byref(a), C.byref(a)) == E_ARG, (sn, dn, i)
        with pytest.raises(ValueError):
            pjd_amd.resize_tap(sn, dn, i)
    assert L.pjd_resize_tap(5, 5, 4, None, None, None) == 0
    assert pjd_amd.resize_tap(65535, 65535, 65534) == (65534, 65534, 0)
    assert pjd_amd.resize_tap(2, 4, 1) == (0, 1, 64)        # centre 0.25: weight 0.25 of sample 1


SHAPES = [(61, 45, 224, 224), (640, 480, 224, 224), (500, 375, 256, 192), (1, 1, 7, 5), (17, 9, 1, 1), (8, 8, 8, 8),
          (300, 200, 299, 199), (33, 77, 64, 3), (2, 2, 255, 255), (447, 335, 224, 224)]


def _pictures(sw, sh, seed):
    rng = np.random.default_rng(seed)
    yield "random", rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    # worst cases for weight quantisation: full-swing stripes and a checkerboard (every tap pair is 0 / 255)
    yy, xx = np.mgrid[0:sh, 0:sw]
    for name, m in (("columns", xx & 1), ("rows", yy & 1), ("checker", (xx + yy) & 1)):
        yield name, np.repeat((m * 255).astype(np.uint8)[..., None], 3, axis=2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_model_within_one_level_of_float64_bilinear(shape):
    """Bound 1 (include/pjd.h): each quantised weight is off by at most 1/512, under 0.4981 levels per axis, under 0.9962 before the one
    rounding; two roundings of values less than 0.9962 apart differ by at most 1."""
    sw, sh, tw, th = shape
    for name, pic in _pictures(sw, sh, sw * 7 + th):
        got = resize_model.resize(pic, tw, th).astype(np.int64)
        assert got.shape == (th, tw, 3)
        exact = resize_model.bilinear_f64(pic, tw, th)
        want = np.floor(exact + 0.5).astype(np.int64)
        worst = int(np.abs(got - want).max())
        print(shape, name, "worst difference to rounded float64 bilinear:", worst, "to the unrounded value: %.4f" % np.abs(got - exact).max())
        assert worst <= 1, (shape, name, worst)
        if (sw, sh) == (tw, th):
            assert np.array_equal(got, pic), "the identity target must reproduce the source"


def test_pick_scale_flags_is_its_rule():
    from pjd_amd import tensors
    dims = [1, 2, 7, 8, 9, 15, 16, 17, 223, 224, 225, 447, 448, 449, 500, 895, 896, 1791, 1792, 1793, 4000]
    targets = [1, 2, 7, 112, 224, 225, 256, 500, 5000]
    for w in dims:
        for h in dims:
            for tw in targets:
                for th in targets:
                    best = 1
                    for s in (1, 2, 4, 8):
                        if -(-w // s) >= tw and -(-h // s) >= th:
                            best = s
                    want = {1: 0, 2: 16, 4: 32, 8: 48}[best]
                    if tw > w or th > h:
                        want = 0
                    got = tensors.pick_scale_flags(w, h, tw, th)
                    assert got == want, (w, h, tw, th, got, want)
                    if w >= tw and h >= th and best < 8:  # the bilinear step then shrinks by less than 2x on the axis that stopped s
                        assert -(-w // best) < 2 * tw or -(-h // best) < 2 * th, (w, h, tw, th)


def test_prescaled_descriptor_copies_leave_the_callers_untouched():
    import pjd_amd
    from pjd_amd import tensors
    from conftest import golden_bytes
    sc = [pjd_amd.Scanned(golden_bytes(n)) for n in ("big_640x480_420_q85", "env_61x45_422_q30", "ilsvrc_val_00000001")]
    sc[1].desc.flags = int(sc[1].desc.flags) | pjd_amd.F_SCALE_1_8 | pjd_amd.F_STANDARD_RESTART
    before = [bytes(C.string_at(C.byref(s.desc), C.sizeof(pjd_amd.ImageDesc))) for s in sc]
    copies = tensors.prescaled_descs([s.desc for s in sc], (224, 224))
    assert [bytes(C.string_at(C.byref(s.desc), C.sizeof(pjd_amd.ImageDesc))) for s in sc] == before
    assert int(copies[0].flags) & pjd_amd.F_SCALE_MASK == pjd_amd.F_SCALE_1_2          # 640x480 -> 320x240 >= 224x224
    assert int(copies[1].flags) & pjd_amd.F_SCALE_MASK == 0 and int(copies[1].flags) & pjd_amd.F_STANDARD_RESTART   # 61x45: smaller than the target
    assert int(copies[2].flags) & pjd_amd.F_SCALE_MASK == tensors.pick_scale_flags(sc[2].desc.width, sc[2].desc.height, 224, 224)
    for s, c in zip(sc, copies):
        assert c is not s.desc and int(c.width) == int(s.desc.width) and int(c.ecs_len) == int(s.desc.ecs_len) and c.ecs == s.desc.ecs
