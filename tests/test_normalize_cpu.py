"""Normalised float output on the host (no GPU): pjd_normalize_value -- the fma the kernel runs, and the conversions include/pjd.h
specifies -- against tests/normalize_model.py for all 256 levels, the three element types and constants that reach subnormals,
infinities and negative values; that the constants used can tell a fused from an unfused implementation; the error returns; the pure
helpers of pjd_amd.tensors."""
import ctypes as C

import numpy as np
import pytest

import normalize_model as nm

E_ARG = -3
DTYPES = [nm.DT_F16, nm.DT_BF16, nm.DT_F32]


@pytest.fixture(scope="module")
def sets():
    from pjd_amd import tensors
    return nm.constant_sets(tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD))


def _lib_table(dtype, scale, bias):
    import pjd_amd
    L = pjd_amd.dev_lib()
    out = np.zeros(256, nm.NP_TYPE[dtype])
    for v in range(256):
        assert L.pjd_normalize_value(dtype, v, C.c_float(scale), C.c_float(bias), C.c_void_p(out[v:].ctypes.data)) == 0
    return out


def test_exports_exist_and_the_abi_version_is_unchanged():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_batch_set_normalize") and hasattr(L, "pjd_normalize_value")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert (pjd_amd.DT_F16, pjd_amd.DT_BF16, pjd_amd.DT_F32) == (1, 2, 3) == (nm.DT_F16, nm.DT_BF16, nm.DT_F32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["imagenet", "unit", "subnormal", "overflow", "negative"])
def test_all_levels_equal_the_model_bit_for_bit(sets, name, dtype):
    scale, bias = sets[name]
    for c in range(3):
        got, want = _lib_table(dtype, scale[c], bias[c]), nm.table(dtype, scale[c], bias[c])
        bad = np.flatnonzero(nm.bits(got) != nm.bits(want))
        assert bad.size == 0, (name, dtype, c, [(int(v), hex(int(nm.bits(got)[v])), hex(int(nm.bits(want)[v]))) for v in bad[:4]])


def test_the_constant_sets_reach_what_they_are_for(sets):
    """64 binary16 subnormals (level 0: zero), infinities of both signs, negative values and a negative zero."""
    h = nm.bits(nm.table(nm.DT_F16, *[a[0] for a in sets["subnormal"]]))
    assert int(np.count_nonzero((h & 0x7c00) == 0)) == 64 and int(np.count_nonzero(h == 0)) == 1
    assert np.all(nm.table(nm.DT_F32, *[a[0] for a in sets["subnormal"]])[1:] >= np.finfo(np.float32).tiny)      # binary32 normals
    over = [nm.bits(nm.table(nm.DT_F16, sets["overflow"][0][c], sets["overflow"][1][c])) for c in range(3)]
    assert np.all(over[0][66:] == 0x7c00) and over[0][65] != 0x7c00 and np.all(over[2][66:] == 0xfc00)
    assert not np.any(np.isinf(nm.table(nm.DT_F32, sets["overflow"][0][0], sets["overflow"][1][0])))
    neg = nm.table(nm.DT_F32, sets["negative"][0][2], sets["negative"][1][2])
    assert nm.bits(neg)[0] == 0x80000000 and np.all(neg[1:] < 0)


def test_the_imagenet_constants_tell_fused_from_unfused_arithmetic(sets):
    """A float32 multiply followed by a float32 add rounds twice: with these constants it differs from the fma on at least 100 of the
    256 levels in every channel at PJD_DT_F32 -- and on none at PJD_DT_F16, so the F32 cases are what pins the fused form."""
    scale, bias = sets["imagenet"]
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        unfused = (v * scale[c]).astype(np.float32) + bias[c]
        assert unfused.dtype == np.float32
        fused = nm.table_f32(scale[c], bias[c])
        n = int(np.count_nonzero(nm.bits(unfused) != nm.bits(fused)))
        print(f"channel {c}: fused and unfused binary32 differ on {n} of 256 levels")
        assert n >= 100, (c, n)
        assert np.array_equal(nm.bits(unfused.astype(np.float16)), nm.bits(fused.astype(np.float16))), c
        assert np.array_equal(nm.bits(_lib_table(nm.DT_F32, scale[c], bias[c])), nm.bits(fused)), c


def test_bf16_of_the_model_is_torch_s_conversion(sets):
    torch = pytest.importorskip("torch")
    for name, (scale, bias) in sets.items():
        for c in range(3):
            u = nm.table_f32(scale[c], bias[c])
            want = torch.tensor(u).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(nm.to_bf16_bits(u), want), (name, c)


def test_model_rounds_once():
    """The rational model against a case where a float64 sum rounded to float32 goes wrong: the exact value lies just above the
    midpoint of two floats, the float64 sum lands on the midpoint and ties to even."""
    from fractions import Fraction
    x = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)          # just above the midpoint of 1 and 1 + 2^-23
    assert nm.round_to_f32(x) == np.float32(1 + 2.0 ** -23)
    assert np.float32(float(x)) == np.float32(1.0)                          # the double rounding the model avoids
    assert nm.round_to_f32(Fraction(1) + Fraction(1, 2 ** 24)) == np.float32(1.0)                   # a tie: to even
    assert nm.round_to_f32(Fraction(1) + Fraction(3, 2 ** 24)) == np.float32(1 + 2.0 ** -22)        # a tie: to even, upwards
    assert nm.round_to_f32(Fraction(2) ** 128) == np.float32(np.inf)
    assert nm.round_to_f32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) == np.finfo(np.float32).max


def test_normalize_value_error_returns():
    import pjd_amd
    L = pjd_amd.dev_lib()
    buf = (C.c_uint8 * 8)(*([0xA5] * 8))
    f = C.c_float
    assert L.pjd_normalize_value(nm.DT_F32, 255, f(1.0), f(0.0), buf) == 0 and bytes(buf) == np.float32(255).tobytes() + b"\xa5" * 4
    buf = (C.c_uint8 * 8)(*([0xA5] * 8))
    assert L.pjd_normalize_value(nm.DT_F16, 1, f(1.0), f(0.0), buf) == 0 and bytes(buf) == b"\x00\x3c" + b"\xa5" * 6      # two bytes, no more
    for bad_dt in (0, 4, -1, 255):
        assert L.pjd_normalize_value(bad_dt, 1, f(1.0), f(0.0), buf) == E_ARG
    assert L.pjd_normalize_value(nm.DT_F16, 256, f(1.0), f(0.0), buf) == E_ARG
    assert L.pjd_normalize_value(nm.DT_F16, 2 ** 32 - 1, f(1.0), f(0.0), buf) == E_ARG
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert L.pjd_normalize_value(nm.DT_F32, 1, f(bad), f(0.0), buf) == E_ARG
        assert L.pjd_normalize_value(nm.DT_F32, 1, f(1.0), f(bad), buf) == E_ARG
    assert L.pjd_normalize_value(nm.DT_F32, 1, f(1.0), f(0.0), None) == E_ARG
    assert bytes(buf)[2:] == b"\xa5" * 6
    with pytest.raises(ValueError):
        pjd_amd.normalize_value(nm.DT_F16, 256, 1.0, 0.0)
    assert pjd_amd.normalize_value(nm.DT_BF16, 1, 1.0, 0.0) == 0x3f80


def test_normalize_constants_is_pure_and_rounds_once():
    from pjd_amd import tensors
    mean, std = list(nm.IMAGENET_MEAN), list(nm.IMAGENET_STD)
    scale, bias = tensors.normalize_constants(mean, std)
    assert mean == list(nm.IMAGENET_MEAN) and std == list(nm.IMAGENET_STD)
    assert scale.dtype == np.float32 and bias.dtype == np.float32 and scale.shape == (3,) and bias.shape == (3,)
    for c in range(3):
        assert scale[c] == np.float32(1.0 / (255.0 * std[c])) and bias[c] == np.float32(-mean[c] / std[c])
    again = tensors.normalize_constants(tuple(mean), np.asarray(std))
    assert np.array_equal(again[0], scale) and np.array_equal(again[1], bias)
    for bad in (([0.5, 0.5], std), (mean, [0.2, 0.0, 0.2]), (mean, [0.2, float("nan"), 0.2])):
        with pytest.raises(ValueError):
            tensors.normalize_constants(*bad)


def test_decode_normalized_batch_tensor_refuses_an_empty_batch_before_touching_the_context():
    from pjd_amd import tensors
    with pytest.raises(ValueError):
        tensors.decode_normalized_batch_tensor(None, [], (224, 224), nm.IMAGENET_MEAN, nm.IMAGENET_STD)


def test_conversions_over_many_binary32_values():
    """v = 1, bias = 0 makes u the scale itself: the two conversions of pjd_normalize_value over 20 000 seeded binary32 values of every
    magnitude (binary16 subnormals, ties, the overflow threshold) against numpy's binary16 and the header's bfloat16 formula."""
    import pjd_amd
    L = pjd_amd.dev_lib()
    rng = np.random.default_rng(16)
    x = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x33000000, 0x33000001, 0x337fffff, 0x33800000, 0x387fc000, 0x387fe000, 0x38800000, 0x477fe000, 0x477fefff, 0x477ff000,
                     0x3f801000, 0x3f803000, 0x3f801001, 0x00000001, 0x007fffff, 0x80000000, 0x7f7fffff, 0xb8000000], np.uint32)
    x = np.concatenate([x, edge, rng.integers(0x33000000, 0x47800000, 8000, dtype=np.uint64).astype(np.uint32)])
    x = x[(x & 0x7f800000) != 0x7f800000].view(np.float32)                  # finite
    h, bf = np.zeros(x.size, np.uint16), np.zeros(x.size, np.uint16)
    for i, f in enumerate(x):
        assert L.pjd_normalize_value(nm.DT_F16, 1, C.c_float(f), C.c_float(0.0), C.c_void_p(h[i:].ctypes.data)) == 0
        assert L.pjd_normalize_value(nm.DT_BF16, 1, C.c_float(f), C.c_float(0.0), C.c_void_p(bf[i:].ctypes.data)) == 0
    u = x + np.float32(0.0)                                                 # fma(1, x, +0): x, but -0 + +0 = +0
    with np.errstate(over="ignore"):
        assert np.array_equal(h, nm.bits(u.astype(np.float16)))
    assert np.array_equal(bf, nm.to_bf16_bits(u))
