"""A per-pixel model of the affine warp of include/pjd.h (pjd_batch_set_resize_affine) in Python integers.  It takes nothing from the
library: the quantisation is Fraction arithmetic on the double's exact value, the rest is `int`.

    quantise(m)                     the six Q40 coefficients, round to nearest even
    tap(m, i, j)                    (x0, y0, wx, wy) of target pixel (column i, row j)
    warp(P, m, tw, th, fill)        P: uint8 [C, sh, sw] -> uint8 [C, th, tw]
    warp_float64(P, m, tw, th, fill) the same filter in float64 with per-tap fill, rounded to nearest (the yardstick of the error bound)
"""
from fractions import Fraction

import numpy as np

Q = 40
LIN_MAX = 16 << Q
SHIFT_MAX = (1 << 18) << Q


def _rint_even(fr):
    fl = fr.numerator // fr.denominator
    rem = fr - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2):
        fl += 1
    return fl


def quantise(m):
    """a = llrint(m * 2^40) for the six values; ValueError where the header refuses the matrix"""
    a = []
    for k, v in enumerate(m):
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")):
            raise ValueError("not finite")
        q = _rint_even(Fraction(v) * (1 << Q))
        if abs(q) > (SHIFT_MAX if k in (2, 5) else LIN_MAX):
            raise ValueError("beyond the limits")
        a.append(q)
    return a


def _wrap64(x):
    """two's complement, 64 bits (the limits keep every sum inside, so this is the identity on accepted matrices)"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def tap(m, i, j):
    a = quantise(m)
    out = []
    for r in (0, 1):
        X = _wrap64(a[3 * r] * (2 * i + 1) + a[3 * r + 1] * (2 * j + 1) + 2 * a[3 * r + 2] - (1 << Q))
        f = (X + (1 << 32)) >> 33
        out.append((f >> 8, f & 255))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def warp(P, m, tw, th, fill=(0, 0, 0)):
    P = np.asarray(P)
    C, sh, sw = P.shape
    a = quantise(m)
    # the positions of all pixels at once, in Python integers (object arrays): exact
    ii = np.arange(tw, dtype=object)[None, :] * 2 + 1
    jj = np.arange(th, dtype=object)[:, None] * 2 + 1
    out = np.empty((C, th, tw), np.uint8)
    fx = (a[0] * ii + a[1] * jj + (2 * a[2] - (1 << Q)) + (1 << 32)) >> 33
    fy = (a[3] * ii + a[4] * jj + (2 * a[5] - (1 << Q)) + (1 << 32)) >> 33
    x0 = (fx >> 8).astype(np.int64); wx = (fx & 255).astype(np.int64)
    y0 = (fy >> 8).astype(np.int64); wy = (fy & 255).astype(np.int64)

    def sample(c, x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        v = P[c][np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64)
        return np.where(inside, v, int(fill[c]))

    for c in range(C):
        s00, s01 = sample(c, x0, y0), sample(c, x0 + 1, y0)
        s10, s11 = sample(c, x0, y0 + 1), sample(c, x0 + 1, y0 + 1)
        top = (256 - wx) * s00 + wx * s01
        bot = (256 - wx) * s10 + wx * s11
        out[c] = (((256 - wy) * top + wy * bot + 32768) >> 16).astype(np.uint8)
    return out


def warp_scalar(P, m, tw, th, fill=(0, 0, 0)):
    """the same, pixel by pixel through tap(): slow, for small pictures (holds warp() and tap() together)"""
    P = np.asarray(P)
    C, sh, sw = P.shape
    out = np.empty((C, th, tw), np.uint8)
    for j in range(th):
        for i in range(tw):
            x0, y0, wx, wy = tap(m, i, j)
            for c in range(C):
                s = [int(P[c, y, x]) if 0 <= x < sw and 0 <= y < sh else int(fill[c]) for y in (y0, y0 + 1) for x in (x0, x0 + 1)]
                out[c, j, i] = ((256 - wy) * ((256 - wx) * s[0] + wx * s[1]) + wy * ((256 - wx) * s[2] + wx * s[3]) + 32768) >> 16
    return out


def warp_float64(P, m, tw, th, fill=(0, 0, 0)):
    P = np.asarray(P)
    C, sh, sw = P.shape
    m = [float(v) for v in m]
    i = np.arange(tw, dtype=np.float64)[None, :] + 0.5
    j = np.arange(th, dtype=np.float64)[:, None] + 0.5
    u = m[0] * i + m[1] * j + m[2] - 0.5
    v = m[3] * i + m[4] * j + m[5] - 0.5
    x0 = np.floor(u); y0 = np.floor(v)
    ax = u - x0; ay = v - y0
    x0 = x0.astype(np.int64); y0 = y0.astype(np.int64)
    out = np.empty((C, th, tw), np.float64)

    def sample(c, x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        val = P[c][np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.float64)
        return np.where(inside, val, float(fill[c]))

    for c in range(C):
        top = (1 - ax) * sample(c, x0, y0) + ax * sample(c, x0 + 1, y0)
        bot = (1 - ax) * sample(c, x0, y0 + 1) + ax * sample(c, x0 + 1, y0 + 1)
        out[c] = (1 - ay) * top + ay * bot
    return out


def similarity(rng, sw, sh, tw, th):
    """a seeded inverse map: rotation by any angle, scale 0.3 .. 3, a translation, about the two centres"""
    ang = rng.uniform(0, 2 * np.pi)
    s = rng.uniform(0.3, 3.0)
    c, sn = np.cos(ang) * s, np.sin(ang) * s
    tx, ty = rng.uniform(-0.3, 0.3) * sw, rng.uniform(-0.3, 0.3) * sh
    return [c, -sn, sw / 2 + tx - c * tw / 2 + sn * th / 2, sn, c, sh / 2 + ty - sn * tw / 2 - c * th / 2]
