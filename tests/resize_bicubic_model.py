"""A numpy model of the bicubic resize, written from the text of include/pjd.h (PJD_RESIZE_BICUBIC, "THE ARITHMETIC"), not from the C
code: raw(sn, dn, i, j) and taps(sn, dn, i) for one target sample of an axis, in Python integers (r_j * 2^17 passes 64 bits on long
axes); axis_taps(sn, dn) for a whole axis as arrays; resize(rgb, tw, th) for a picture, with the accumulator bounds of the header
asserted; cubic_f64, the same filter with exact weights in float64, neither clamped nor rounded (what
torch.nn.functional.interpolate(mode="bicubic", antialias=True) computes on a float64 tensor)."""
import functools

import numpy as np

MAX_TAPS = 64
MAX_GAIN = 92681


def raw(sn, dn, i, j):
    """(D, T, r_j) of source sample j for target sample i: exact integers; r_j is None outside the support (D >= 2 * T)."""
    sn, dn, i, j = int(sn), int(dn), int(i), int(j)
    T = 2 * max(sn, dn)
    D = abs((2 * j + 1) * dn - (2 * i + 1) * sn)
    if D < T:
        return D, T, 3 * D ** 3 - 5 * T * D ** 2 + 2 * T ** 3
    if D < 2 * T:
        return D, T, -D ** 3 + 5 * T * D ** 2 - 8 * T ** 2 * D + 4 * T ** 3
    return D, T, None


def taps(sn, dn, i):
    """(first, [q ...]): the run of source samples inside the support -- whatever their weight -- quantised to 1/65536 with floor
    division (round half up, either sign) and corrected to sum to 65536."""
    sn, dn, i = int(sn), int(dn), int(i)
    S = max(sn, dn)
    # candidates: a window of source samples that surely holds every j with D < 4 * S (two spare on either side)
    j0 = max(0, ((2 * i + 1) * sn - 4 * S) // (2 * dn) - 2)
    cand = [(j, raw(sn, dn, i, j)[2]) for j in range(j0, min(sn, j0 + -(-4 * S // dn) + 6))]
    assert cand[0][1] is None or cand[0][0] == 0, "the window starts before the support, or at sample 0"
    assert cand[-1][1] is None or cand[-1][0] == sn - 1, "the window ends behind the support, or at the last sample"
    run = [(j, r) for j, r in cand if r is not None]
    first, r = run[0][0], [v for _, v in run]
    assert [j for j, _ in run] == list(range(first, first + len(r))), "the taps are one run"
    R = sum(r)
    assert R > 0
    q = [(2 * 65536 * v + R) // (2 * R) for v in r]          # Python's // rounds down for either sign
    q[r.index(max(r))] += 65536 - sum(q)                     # list.index: the lowest j on a tie
    return first, q


@functools.lru_cache(maxsize=256)
def _axis_taps(sn, dn):
    per = [taps(sn, dn, i) for i in range(dn)]
    first = np.array([f for f, _ in per], dtype=np.int64)
    count = np.array([len(q) for _, q in per], dtype=np.int64)
    q = np.zeros((dn, int(count.max())), dtype=np.int64)
    for i, (_, w) in enumerate(per):
        q[i, :len(w)] = w
    for a in (first, count, q):
        a.setflags(write=False)
    return first, count, q


def axis_taps(sn, dn):
    """(first[dn], count[dn], q[dn][n]) as int64 arrays, n the largest count of the axis, q zero behind a sample's own count."""
    return _axis_taps(int(sn), int(dn))


def gain(sn, dn):
    """The largest sum |q_j| over the target samples of the axis (A of include/pjd.h for this axis)."""
    return int(np.abs(axis_taps(sn, dn)[2]).sum(axis=1).max())


def _apply(first, q, a):
    """Filter axis 0 of `a` (sn x ...) -> dn x ...: sum_t q[i, t] * a[first[i] + t]."""
    out = np.zeros((len(first),) + a.shape[1:], dtype=np.int64)
    for t in range(q.shape[1]):
        w = q[:, t].reshape((-1,) + (1,) * (a.ndim - 1))
        out += w * a[np.minimum(first + t, a.shape[0] - 1)]          # past the count the weight is 0
    return out


def resize(rgb, tw, th, stats=None):
    """H x W x 3 uint8 -> th x tw x 3 uint8.  stats (a dict): receives how many samples the one clamp caught below 0 and above 255,
    and "pre", the value before the final rounding and clamp (v / 2^22, float64)."""
    P = np.asarray(rgb).astype(np.int64)
    sh, sw, _ = P.shape
    fx, _, qx = axis_taps(sw, tw)
    fy, _, qy = axis_taps(sh, th)
    A = max(int(np.abs(qx).sum(axis=1).max()), int(np.abs(qy).sum(axis=1).max()))
    assert A <= MAX_GAIN and max(np.abs(qx).max(), np.abs(qy).max()) < 1 << 18
    h = _apply(fx, qx, P.transpose(1, 0, 2)).transpose(1, 0, 2)      # sh x tw x 3, signed
    assert np.abs(h).max() <= 255 * A < 1 << 31
    h6 = (h + 512) >> 10                                   # numpy's >> on int64 is arithmetic
    assert np.abs(h6).max() <= 23080 < 1 << 15
    v = _apply(fy, qy, h6)
    assert np.abs(v).max() + (1 << 21) < 1 << 31
    out = (v + (1 << 21)) >> 22
    if stats is not None:
        stats["below"] = stats.get("below", 0) + int((out < 0).sum())
        stats["above"] = stats.get("above", 0) + int((out > 255).sum())
        stats["pre"] = v / float(1 << 22)
    return np.clip(out, 0, 255).astype(np.uint8)


def keys(x):
    """Keys' cubic convolution kernel with a = -0.5."""
    x = np.abs(x)
    return np.where(x < 1, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2, ((-0.5 * x + 2.5) * x - 4) * x + 2, 0.0))


def axis_f64(sn, dn):
    """The exact weights of an axis, dn x sn float64: half-pixel centres, support 2 target samples where the axis grows or stays and
    2 * sn / dn source samples where it shrinks, clipped to the picture and renormalised."""
    scale = max(sn / dn, 1.0)
    centre = (np.arange(dn) + 0.5) * sn / dn               # in source pixels, sample j at j + 0.5
    j = np.arange(sn) + 0.5
    w = keys((j[None, :] - centre[:, None]) / scale)
    return w / w.sum(axis=1, keepdims=True)


def horizontal_f64(rgb, tw):
    """The horizontal pass alone in float64: sh x tw x 3."""
    P = np.asarray(rgb).astype(np.float64)
    return np.einsum("xj,yjc->yxc", axis_f64(P.shape[1], tw), P)


def cubic_f64(rgb, tw, th):
    """The unquantised separable filter: float64 result, neither clamped nor rounded."""
    sh = np.asarray(rgb).shape[0]
    return np.einsum("iy,yxc->ixc", axis_f64(sh, th), horizontal_f64(rgb, tw))
