"""The colour map of include/pjd.h (pjd_batch_set_colour, section "colour map") in Python integers: the quantisation, the limits and
the one-clamp arithmetic, sample by sample (value) and over whole arrays (apply, numpy int64: no sum of the header can wrap there
either).  The tests hold the library against it; nothing here is computed by the library."""
import math

import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
Q_LIMIT, O_LIMIT = 1 << 20, 1 << 28


def rint_even(x):
    """llrint of a finite float in the default rounding mode: to nearest, ties to even -- exactly, through the float's own fraction"""
    n, d = float(x).as_integer_ratio()
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q


def quantise(m):
    """[q00, q01, q02, o0, q10, ...]: twelve integers, or ValueError where the header refuses the matrix"""
    m = [float(v) for row in m for v in (row if hasattr(row, "__len__") else (row,))]
    if len(m) != 12:
        raise ValueError("twelve values")
    out = []
    for k, v in enumerate(m):
        if not math.isfinite(v):
            raise ValueError("not finite")
        q = rint_even(v * 65536.0)                          # a product with a power of two: exact (or an overflow to inf, refused above 1e300 / 65536)
        if abs(q) > (O_LIMIT if k % 4 == 3 else Q_LIMIT):
            raise ValueError("beyond the limits")
        out.append(q)
    return out


def check(m):
    try:
        quantise(m)
        return True
    except (ValueError, OverflowError):
        return False


def is_identity(m):
    return quantise(m) == [65536 if k in (0, 5, 10) else 0 for k in range(12)]


def value(m, rgb):
    q = quantise(m)
    r, g, b = (int(v) for v in rgb)
    out = []
    for c in range(3):
        s = q[4 * c] * r + q[4 * c + 1] * g + q[4 * c + 2] * b + q[4 * c + 3] + 32768
        assert -(1 << 31) <= s < (1 << 31)
        out.append(min(max(s >> 16, 0), 255))              # Python's >> on a negative int is the arithmetic shift
    return tuple(out)


def apply(m, chw):
    """the map over a uint8 picture [3, ...] -> uint8 of the same shape"""
    q = np.asarray(quantise(m), np.int64).reshape(3, 4)
    p = np.asarray(chw).astype(np.int64)
    assert p.shape[0] == 3
    s = np.stack([q[c, 0] * p[0] + q[c, 1] * p[1] + q[c, 2] * p[2] + q[c, 3] + 32768 for c in range(3)])
    return np.clip(s >> 16, 0, 255).astype(np.uint8)


def float64(m, chw):
    """the same map in float64, unrounded and clamped: what the header's error bound is stated against"""
    a = np.asarray([float(v) for v in m], np.float64).reshape(3, 4)
    p = np.asarray(chw).astype(np.float64)
    x = np.stack([a[c, 0] * p[0] + a[c, 1] * p[1] + a[c, 2] * p[2] + a[c, 3] for c in range(3)])
    return np.clip(x, 0.0, 255.0)


def permutation(order):
    """out[c] = in[order[c]]"""
    m = [0.0] * 12
    for c, k in enumerate(order):
        m[4 * c + k] = 1.0
    return tuple(m)


def jitter(rng):
    """a seeded ColorJitter-like matrix within the limits: a random linear part around the identity and an offset"""
    lin = np.eye(3) * rng.uniform(0.4, 1.8) + rng.uniform(-0.6, 0.6, (3, 3))
    off = rng.uniform(-90, 90, 3)
    return tuple(float(v) for v in np.concatenate([lin, off[:, None]], axis=1).reshape(-1))
