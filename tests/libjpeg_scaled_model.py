"""libjpeg_scaled_model.py -- numpy restatement of the arithmetic of PJD_F_LIBJPEG_SCALE_* (include/pjd.h, "libjpeg-exact REDUCED-SIZE
decode"), written from that text alone: the size of each component's IDCT, the 4x4, 2x2 and 1x1 transforms, what is left of the
upsampling.  Everything is int32 that wraps, as numpy's is.  The full-size transform, the h2v1 fancy row, the colour tables and the
coefficient layout are those of tests/libjpeg_model.py (the full-size section of the same header).
"""
import numpy as np

import libjpeg_model as M

I32 = np.int32


def chroma_size(n, hs, vs):
    """Samples a side of a chroma unit where a luma unit has n: doubles while cn < 8, 2*cn <= hs*n and 2*cn <= vs*n."""
    cn = n
    while cn < 8 and 2 * cn <= hs * n and 2 * cn <= vs * n:
        cn *= 2
    return cn


def _round(v, sh):
    return (v + I32(1 << (sh - 1))) >> I32(sh)


def _k4(i, sh):
    """The 4x4 1-D kernel: reads i0, i1, i2, i3, i5, i6, i7."""
    i0, i1, i2, i3, _, i5, i6, i7 = i
    c = I32
    t0 = i0 << c(14)
    t2 = i2 * c(15137) - i6 * c(6270)
    t10, t12 = t0 + t2, t0 - t2
    a0 = -i7 * c(1730) + i5 * c(11893) - i3 * c(17799) + i1 * c(8697)
    a2 = -i7 * c(4176) - i5 * c(4926) + i3 * c(7373) + i1 * c(20995)
    return [_round(v, sh) for v in (t10 + a2, t12 + a0, t12 - a0, t10 - a2)]


def _k2(i, sh):
    """The 2x2 1-D kernel: reads i0, i1, i3, i5, i7."""
    i0, i1, _, i3, _, i5, _, i7 = i
    c = I32
    t10 = i0 << c(15)
    t0 = -i7 * c(5906) + i5 * c(6967) - i3 * c(10426) + i1 * c(29692)
    return [_round(v, sh) for v in (t10 + t0, t10 - t0)]


def idct_units(coef, q, n):
    """coef int16 [..., 64], q [64] in natural order -> uint8 samples [..., n, n], n = 8, 4, 2 or 1."""
    coef = np.asarray(coef)
    if n == 8:
        return M.idct_units(coef, q)
    with np.errstate(over="ignore"):
        d = (coef.astype(I32) * np.asarray(q).astype(np.int64).astype(I32)).reshape(coef.shape[:-1] + (8, 8))
        if n == 1:
            out = ((d[..., 0, 0] + I32(4)) >> I32(3))[..., None, None]
        else:
            k, s1, s2 = (_k4, 12, 19) if n == 4 else (_k2, 13, 20)
            # pass 1: per column (the skipped columns are computed too and never read), rows as inputs -> workspace [n rows, 8 columns]
            ws = np.stack(k([d[..., j, :] for j in range(8)], s1), axis=-2)
            # pass 2: per workspace row, columns as inputs -> n samples
            out = np.stack(k([ws[..., :, j] for j in range(8)], s2), axis=-1)
        return np.clip(out.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def plane_from_units(samples):
    """[uy, ux, n, n] -> [uy * n, ux * n]."""
    uy, ux, n, _ = samples.shape
    return samples.transpose(0, 2, 1, 3).reshape(uy * n, ux * n)


def out_size(width, height, s):
    return (width + s - 1) // s, (height + s - 1) // s


def decode(coef, qts, width, height, ncomp, hs, vs, s, gray=False):
    """The picture P of a flagged descriptor at scale 1/s (s = 1, 2, 4, 8): [oh, ow, 3], or the luma plane [oh, ow] with gray=True.
    coef in the download layout (M.unit_grids), qts[c] the 64 quantisers of component c in natural order."""
    n = 8 // s
    ow, oh = out_size(width, height, s)
    if s == 1 and not gray:
        return M.decode(coef, qts, width, height, ncomp, hs, vs)     # the full-size section: h2v2 upsampling exists only there
    grids = M.unit_grids(coef, width, height, ncomp, hs, vs)
    yp = plane_from_units(idct_units(grids[0], np.asarray(qts[0]).reshape(64), n))[:oh, :ow]
    if gray:
        return yp
    if ncomp == 1:
        return np.stack([yp, yp, yp], axis=-1)
    cn = chroma_size(n, hs, vs)
    ch = []
    for c in (1, 2):
        p = plane_from_units(idct_units(grids[c], np.asarray(qts[c]).reshape(64), cn))
        if cn == n * hs and cn == n * vs:
            ch.append(p[:oh, :ow])                  # sample for sample: 4:4:4, and 4:2:0 whose chroma transform doubled
            continue
        assert (hs, vs) == (2, 1) and cn == n       # h2v1 is all the upsampling that is left
        dw, dh = -(-width * cn // 16), -(-height * cn // 8)
        assert dh == oh and dw == (ow + 1) // 2
        p = p[:dh, :dw]
        if n > 1:                                   # fancy where dw > 2 (M.upsample_row replicates at dw <= 2)
            up = np.stack([M.upsample_row(r) for r in p])
        else:                                       # 1/8: libjpeg switches fancy upsampling off at min_DCT_scaled_size 1
            up = np.repeat(p, 2, axis=1)
        ch.append(up[:, :ow])
    return M.ycc_to_rgb(yp, ch[0], ch[1])
