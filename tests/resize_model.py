"""A numpy model of the resize-on-decode filter, written from the text of include/pjd.h (pjd_batch_set_resize, "THE ARITHMETIC"),
not from the kernel: taps(sn, dn) for one axis, resize(rgb, tw, th) for a picture, and bilinear_f64, the same filter with exact
weights in float64 (what torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) computes)."""
import numpy as np


def taps(sn, dn):
    """(i0, i1, w) as int64 arrays over the dn target samples of an axis with sn source samples."""
    sn, dn = int(sn), int(dn)
    i = np.arange(dn, dtype=np.int64)
    X = (2 * i + 1) * sn - dn
    X = np.clip(X, 0, 2 * dn * (sn - 1))
    i0 = X // (2 * dn)
    w = ((X - i0 * 2 * dn) * 256 + dn) // (2 * dn)
    i1 = np.minimum(i0 + 1, sn - 1)
    return i0, i1, w


def resize(rgb, tw, th):
    """H x W x 3 uint8 -> th x tw x 3 uint8."""
    P = np.asarray(rgb).astype(np.int64)
    sh, sw, _ = P.shape
    x0, x1, wx = taps(sw, tw)
    y0, y1, wy = taps(sh, th)
    wx = wx[None, :, None]
    wy = wy[:, None, None]
    top = (256 - wx) * P[y0][:, x0] + wx * P[y0][:, x1]
    bot = (256 - wx) * P[y1][:, x0] + wx * P[y1][:, x1]
    out = ((256 - wy) * top + wy * bot + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def bilinear_f64(rgb, tw, th):
    """The unquantised filter: float64 result, not rounded."""
    P = np.asarray(rgb).astype(np.float64)
    sh, sw, _ = P.shape

    def axis(sn, dn):
        c = np.clip((np.arange(dn) + 0.5) * sn / dn - 0.5, 0, sn - 1)
        i0 = np.floor(c).astype(np.int64)
        return i0, np.minimum(i0 + 1, sn - 1), c - i0

    x0, x1, fx = axis(sw, tw)
    y0, y1, fy = axis(sh, th)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    top = (1 - fx) * P[y0][:, x0] + fx * P[y0][:, x1]
    bot = (1 - fx) * P[y1][:, x0] + fx * P[y1][:, x1]
    return (1 - fy) * top + fy * bot
