"""The Gaussian blur of include/pjd.h (pjd_batch_set_blur) as a model: integers over the header's text -- the border rule, the two passes
with their roundings, the limits of the sums asserted on the way -- and the same filter in float64 beside it.  The taps are the
library's own (pjd_amd.blur_taps: the one table the host builds); taps_float is the header's formula in Python floats, what they are held
against.  Pictures are numpy uint8 arrays, one channel [H, W] or planes [C, H, W]; interleaved() takes [H, W, C]."""
import math

import numpy as np

import pjd_amd

MAX_TAPS = 63


def taps(ksize, sigma):
    return pjd_amd.blur_taps(ksize, sigma)


def weights_float(ksize, sigma):
    """w[j] / t of the header, unquantised"""
    r = ksize // 2
    w = [math.exp(-0.5 * ((j - r) / sigma) ** 2) for j in range(ksize)]
    t = 0.0
    for v in w:
        t += v
    return [v / t for v in w]


def taps_float(ksize, sigma):
    """the header's table in Python floats: round half to even (llrint), the remainder into the centre"""
    q = [int(round(v * 65536.0)) for v in weights_float(ksize, sigma)]
    q[ksize // 2] += 65536 - sum(q)
    return q


def index(n, i):
    """the border rule: torchvision's reflect, folded as often as it takes"""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p                                              # Python's remainder: 0 <= m < p
    return m if m < n else p - m


def check(ksize, sigma, reserved=0):
    if reserved != 0:
        return False
    if ksize == 0:
        return sigma == 0
    return ksize % 2 == 1 and ksize <= MAX_TAPS and math.isfinite(sigma) and sigma > 0


def is_identity(q):
    return q[len(q) // 2] == 65536


def _gather(n, r):
    """[n, 2r + 1]: the sample every tap of every output index reads"""
    return np.array([[index(n, i + j - r) for j in range(2 * r + 1)] for i in range(n)], dtype=np.int64)


def blur_plane(u, q):
    """one channel [H, W] through the taps q: horizontal, the row sample, vertical, the final rounding"""
    u = np.asarray(u)
    assert u.dtype == np.uint8 and u.ndim == 2
    hgt, wid = u.shape
    qa, r = np.array(q, dtype=np.int64), len(q) // 2
    assert int(qa.sum()) == 65536 and qa.min() >= 0
    h = (u.astype(np.int64)[:, _gather(wid, r)] * qa).sum(axis=2)
    assert h.max() <= 255 * 65536 < 1 << 24
    h8 = (h + 128) >> 8
    assert h8.max() <= 65280
    v = (h8[_gather(hgt, r), :] * qa[None, :, None]).sum(axis=1)
    assert v.max() + (1 << 23) < 1 << 32
    return ((v + (1 << 23)) >> 24).astype(np.uint8)


def blur(u, entry):
    """[H, W] or [C, H, W] through one entry of set_blur: None or (ksize, sigma)"""
    u = np.asarray(u)
    if entry is None or entry[0] == 0:
        return u.copy()
    q = taps(*entry)
    if u.ndim == 2:
        return blur_plane(u, q)
    return np.stack([blur_plane(p, q) for p in u])


def interleaved(u, entry):
    """[H, W, C]"""
    return np.ascontiguousarray(blur(np.moveaxis(np.asarray(u), 2, 0), entry).transpose(1, 2, 0))


def blur_float(u, entry):
    """the same filter in float64: the unquantised weights, the same border, no rounding anywhere"""
    u = np.asarray(u, dtype=np.float64)
    if entry is None or entry[0] == 0:
        return u.copy()
    if u.ndim == 3:
        return np.stack([blur_float(p, entry) for p in u])
    w, r = np.array(weights_float(*entry)), entry[0] // 2
    hgt, wid = u.shape
    h = (u[:, _gather(wid, r)] * w).sum(axis=2)
    return (h[_gather(hgt, r), :] * w[None, :, None]).sum(axis=1)
