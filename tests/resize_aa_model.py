"""A numpy model of the antialiased resize, written from the text of include/pjd.h (pjd_batch_set_resize_filter, "THE ARITHMETIC"),
not from the C code: taps(sn, dn, i) for one target sample of an axis (every source sample looked at), axis_taps(sn, dn) for a whole
axis (vectorised over a window of candidates; tests/test_resize_aa_cpu.py holds the two together), resize(rgb, tw, th) for a picture, and triangle_f64, the same filter with exact weights in float64 (what torch.nn.functional.interpolate(mode="bilinear",
antialias=True) and Pillow's BILINEAR compute), not rounded."""
import functools

import numpy as np


def raw_weights(sn, dn, i):
    """r_j for every j of 0..sn-1, as Python-exact int64 (the largest value, 2 * 65535 * 65535 + ..., fits)."""
    sn, dn, i = int(sn), int(dn), int(i)
    S = max(sn, dn)
    j = np.arange(sn, dtype=np.int64)
    return np.maximum(0, 2 * S - np.abs((2 * j + 1) * dn - (2 * i + 1) * sn))


def taps(sn, dn, i):
    """(first, [q ...]): the contiguous run of source samples with a raw weight, quantised to 1/65536 and corrected to sum to 65536."""
    r = raw_weights(sn, dn, i)
    nz = np.flatnonzero(r)
    first, count = int(nz[0]), len(nz)
    assert np.array_equal(nz, np.arange(first, first + count)), "the taps are one run"
    r = [int(v) for v in r[first:first + count]]
    R = sum(r)
    q = [(v * 65536 + R // 2) // R for v in r]
    q[r.index(max(r))] += 65536 - sum(q)                   # list.index: the lowest j on a tie
    return first, q


@functools.lru_cache(maxsize=64)
def _axis_taps(sn, dn):
    S = max(sn, dn)
    i = np.arange(dn, dtype=np.int64)[:, None]
    c = (2 * i + 1) * sn
    # candidates: a window of source samples that surely holds every j with |(2j + 1) dn - c| < 2S (two spare on either side)
    j0 = np.maximum(0, (c - 2 * S) // (2 * dn) - 2)
    j = j0 + np.arange(-(-2 * S // dn) + 6, dtype=np.int64)[None, :]
    r = np.where(j < sn, np.maximum(0, 2 * S - np.abs((2 * j + 1) * dn - c)), 0)
    assert not r[:, 0].any() or not j0[r[:, 0] > 0].any(), "the window starts before the first tap, or at sample 0"
    assert not r[:, -1].any()
    lead = (r > 0).argmax(axis=1)                          # candidates before the first tap
    count = (r > 0).sum(axis=1)
    T = int(count.max())
    k = lead[:, None] + np.arange(T)[None, :]
    r = np.take_along_axis(r, k, axis=1)                   # the taps, left-aligned; 0 behind a sample's own count (the run is contiguous)
    assert np.array_equal((r > 0).sum(axis=1), count), "the taps are one run"
    R = r.sum(axis=1, keepdims=True)
    q = (r * 65536 + R // 2) // R
    q[np.arange(dn), r.argmax(axis=1)] += 65536 - q.sum(axis=1)      # argmax: the lowest j on a tie
    first = j0[:, 0] + lead
    for a in (first, count, q):
        a.setflags(write=False)
    return first, count, q


def axis_taps(sn, dn):
    """(first[dn], count[dn], q[dn][T]) as int64 arrays, T the largest count of the axis, q zero behind a sample's own count."""
    return _axis_taps(int(sn), int(dn))


def _apply(first, q, a):
    """Filter axis 0 of `a` (sn x ...) -> dn x ...: sum_t q[i, t] * a[first[i] + t]."""
    out = np.zeros((len(first),) + a.shape[1:], dtype=np.int64)
    for t in range(q.shape[1]):
        w = q[:, t].reshape((-1,) + (1,) * (a.ndim - 1))
        out += w * a[np.minimum(first + t, a.shape[0] - 1)]          # past the count the weight is 0
    return out


def resize(rgb, tw, th):
    """H x W x 3 uint8 -> th x tw x 3 uint8."""
    P = np.asarray(rgb).astype(np.int64)
    sh, sw, _ = P.shape
    fx, _, qx = axis_taps(sw, tw)
    fy, _, qy = axis_taps(sh, th)
    h = _apply(fx, qx, P.transpose(1, 0, 2)).transpose(1, 0, 2)      # sh x tw x 3
    assert h.max() < 1 << 24
    h16 = (h + 128) >> 8
    assert h16.max() <= 65280
    v = _apply(fy, qy, h16)
    assert v.max() < (1 << 32) - (1 << 23)
    out = (v + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def triangle_f64(rgb, tw, th):
    """The unquantised filter: float64 result, not rounded.  Per axis: the triangle with half-pixel centres, support 1 target sample
    where the axis grows or stays and sn/dn source samples where it shrinks, clipped to the picture and renormalised."""
    P = np.asarray(rgb).astype(np.float64)
    sh, sw, _ = P.shape

    def axis(sn, dn):
        scale = max(sn / dn, 1.0)
        centre = (np.arange(dn) + 0.5) * sn / dn           # in source pixels, sample j at j + 0.5
        j = np.arange(sn) + 0.5
        w = np.maximum(0.0, 1.0 - np.abs(j[None, :] - centre[:, None]) / scale)
        return w / w.sum(axis=1, keepdims=True)

    return np.einsum("iy,yxc->ixc", axis(sh, th), np.einsum("xj,yjc->yxc", axis(sw, tw), P))
