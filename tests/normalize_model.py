"""A model of the normalised float output, written from the text of include/pjd.h (pjd_batch_set_normalize, "THE ARITHMETIC"), not
from the kernel: for one (scale, bias) the 256 values u = fma((float)v, scale, bias) are computed with exact rational arithmetic
(fractions.Fraction) and rounded ONCE to binary32, ties to even, by comparing the exact value with the neighbouring floats -- never
through a float64 sum, which would round twice.  binary16 is numpy's conversion (nearest even), bfloat16 the header's bit formula.

    table_f32(scale, bias)               the 256 values of u, np.float32
    table(dtype, scale, bias)            ... converted: np.float16, np.uint16 (bfloat16 bits) or np.float32
    normalize(rgb_u8, dtype, scale, bias)   a [..., 3] uint8 picture through the three tables of its channels
    bits(a)                              an array of any of the three as unsigned integers, for bit-for-bit comparisons
"""
from fractions import Fraction

import numpy as np

DT_F16, DT_BF16, DT_F32 = 1, 2, 3
ESIZE = {DT_F16: 2, DT_BF16: 2, DT_F32: 4}
NP_TYPE = {DT_F16: np.float16, DT_BF16: np.uint16, DT_F32: np.float32}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_F32_MAX = Fraction(int(np.finfo(np.float32).max))
_F32_OVERFLOW = Fraction(2) ** 128 - Fraction(2) ** 103          # max + half an ulp: from here on nearest-even gives infinity


def round_to_f32(x, zero_sign_negative=False):
    """The binary32 nearest to the exact rational x, ties to even."""
    if x == 0:
        return np.float32(-0.0) if zero_sign_negative else np.float32(0.0)
    if abs(x) >= _F32_OVERFLOW:
        return np.float32(np.inf) if x > 0 else np.float32(-np.inf)
    # a first guess (two roundings: possibly one float off), then the exact comparison with it and its two neighbours
    guess = np.float32(min(max(float(x), -float(_F32_MAX)), float(_F32_MAX)))
    with np.errstate(over="ignore"):
        cands = {float(guess), float(np.nextafter(guess, np.float32(np.inf))), float(np.nextafter(guess, np.float32(-np.inf)))}
    best = None
    for c in cands:
        if not np.isfinite(c):
            continue
        d = abs(x - Fraction(c))
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, even, c)
    return np.float32(best[2])


_TABLES = {}


def table_f32(scale, bias):
    s, b = np.float32(scale), np.float32(bias)
    assert np.isfinite(s) and np.isfinite(b)
    key = (int(s.view(np.uint32)), int(b.view(np.uint32)))         # the bits: -0.0 is not 0.0
    if key not in _TABLES:
        _TABLES[key] = _table_f32(s, b)
    return _TABLES[key].copy()


def _table_f32(s, b):
    fs, fb = Fraction(float(s)), Fraction(float(b))
    out = np.zeros(256, np.float32)
    for v in range(256):
        # an exact zero is -0 only when the product and the addend are both negative zeros (IEEE 754, nearest even)
        neg0 = bool(np.signbit(b)) and (bool(np.signbit(s)) if v == 0 or s == 0 else False)
        out[v] = round_to_f32(v * fs + fb, neg0)
    return out


def to_bf16_bits(u):
    bits = np.asarray(u, np.float32).view(np.uint32).astype(np.uint64)
    bits = bits + 0x7fff + ((bits >> 16) & 1)
    return ((bits >> 16) & 0xffff).astype(np.uint16)


def table(dtype, scale, bias):
    u = table_f32(scale, bias)
    if dtype == DT_F32:
        return u
    if dtype == DT_F16:
        with np.errstate(over="ignore"):
            return u.astype(np.float16)
    assert dtype == DT_BF16
    return to_bf16_bits(u)


def normalize(rgb_u8, dtype, scale, bias):
    """[..., 3] uint8 (channel last: R, G, B) -> the same shape in NP_TYPE[dtype]."""
    rgb_u8 = np.asarray(rgb_u8)
    assert rgb_u8.dtype == np.uint8 and rgb_u8.shape[-1] == 3
    out = np.zeros(rgb_u8.shape, NP_TYPE[dtype])
    for c in range(3):
        out[..., c] = table(dtype, scale[c], bias[c])[rgb_u8[..., c]]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def constant_sets(imagenet):
    """The constant sets of the tests, name -> (scale[3], bias[3]) as np.float32; `imagenet`: what
    pjd_amd.tensors.normalize_constants(IMAGENET_MEAN, IMAGENET_STD) returned."""
    f = np.float32
    tiny = f(2.0 ** -20 * (1 + 2.0 ** -10))                        # levels 0..63 give binary16 subnormals (or zero)
    return {
        "imagenet": (np.asarray(imagenet[0], f), np.asarray(imagenet[1], f)),
        "unit": (np.full(3, f(1.0 / 255.0)), np.zeros(3, f)),
        "subnormal": (np.full(3, tiny), np.zeros(3, f)),
        "overflow": (np.array([1000, 1000, -1000], f), np.array([0, 0.5, 0], f)),      # binary16 overflows to +-infinity from level 66 on
        "negative": (np.array([-1.0 / 255.0, -0.0173, -3.5], f), np.array([1.0, 0.25, -0.0], f)),
    }
