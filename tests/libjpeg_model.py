"""libjpeg_model.py -- numpy restatement of the arithmetic of PJD_F_LIBJPEG (include/pjd.h, "libjpeg-exact decode"), written from that
text alone: dequantise, jpeg_idct_islow, fancy upsampling, the JFIF colour tables.  Everything is int32 that wraps, as numpy's is.

Coefficients come in the layout of pjd_batch_download_coefficients / oracle_lib.Port.decode()["coef"] (the reference's MCU_buffer):
flat index blk16 * 768 + component * 256 + position * 64 + natural index.
"""
import numpy as np

I32 = np.int32


def unit_grids(coef, width, height, ncomp, hs, vs):
    """[component] -> int16 array [units down, units across, 64] over the padded MCU grid (component planes of whole MCUs)."""
    flat = np.asarray(coef, np.int16).reshape(-1)
    w8, h8 = (width + 7) // 8, (height + 7) // 8
    wr = w8 + (1 if hs == 2 and w8 % 2 else 0)
    mcux, mcuy = (w8 + hs - 1) // hs, (h8 + vs - 1) // vs

    def unit(comp, y, x):
        m8 = y * wr + x
        blk = (m8 // (2 * wr)) * ((wr + 1) // 2) + (m8 % wr) // 2
        pos = ((m8 // wr) % 2) * 2 + (m8 % wr) % 2
        o = blk * 768 + comp * 256 + pos * 64
        return flat[o:o + 64] if o + 64 <= flat.size else np.zeros(64, np.int16)

    grids = [np.zeros((mcuy * vs, mcux * hs, 64), np.int16)]
    for y in range(mcuy * vs):
        for x in range(mcux * hs):
            grids[0][y, x] = unit(0, y, x)
    for c in range(1, ncomp):
        g = np.zeros((mcuy, mcux, 64), np.int16)
        for y in range(mcuy):
            for x in range(mcux):
                g[y, x] = unit(c, y * vs, x * hs)
        grids.append(g)
    return grids


def _idct1d(i, s):
    """The 1-D kernel on eight int32 arrays, each output (o + (1 << (s - 1))) >> s."""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    c = lambda v: I32(v)
    z1 = (i2 + i6) * c(4433)
    t2 = z1 - i6 * c(15137)
    t3 = z1 + i2 * c(6270)
    t0 = (i0 + i4) << c(13)
    t1 = (i0 - i4) << c(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * c(9633)
    a0, a1, a2, a3 = a0 * c(2446), a1 * c(16819), a2 * c(25172), a3 * c(12299)
    z1, z2 = z1 * c(-7373), z2 * c(-20995)
    z3, z4 = z3 * c(-16069) + z5, z4 * c(-3196) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [(v + c(1 << (s - 1))) >> c(s) for v in o]


def idct_units(coef, q):
    """coef int16 [..., 64], q [64] (or broadcastable) in natural order -> uint8 samples [..., 8, 8]."""
    with np.errstate(over="ignore"):
        d = (np.asarray(coef).astype(I32) * np.asarray(q).astype(np.int64).astype(I32)).reshape(coef.shape[:-1] + (8, 8))
        ws = np.stack(_idct1d([d[..., j, :] for j in range(8)], 11), axis=-2)          # pass 1: columns
        out = np.stack(_idct1d([ws[..., :, j] for j in range(8)], 18), axis=-1)        # pass 2: rows
        return np.clip(out.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def plane_from_units(samples):
    """[uy, ux, 8, 8] -> [uy * 8, ux * 8]."""
    uy, ux = samples.shape[:2]
    return samples.transpose(0, 2, 1, 3).reshape(uy * 8, ux * 8)


def upsample_row(cur, nb=None):
    """One output row of 2n samples from the chroma row `cur` (n samples) and, for h2v2, its neighbour row."""
    cur = np.asarray(cur).astype(np.int64)
    n = cur.size
    if n <= 2:
        return np.repeat(cur, 2).astype(np.uint8)
    out = np.zeros(2 * n, np.int64)
    if nb is None:
        out[0], out[2 * n - 1] = cur[0], cur[n - 1]
        for i in range(n):
            if i > 0:
                out[2 * i] = (3 * cur[i] + cur[i - 1] + 1) >> 2
            if i < n - 1:
                out[2 * i + 1] = (3 * cur[i] + cur[i + 1] + 2) >> 2
    else:
        s = 3 * cur + np.asarray(nb).astype(np.int64)
        out[0], out[2 * n - 1] = (4 * s[0] + 8) >> 4, (4 * s[n - 1] + 7) >> 4
        for i in range(n):
            if i > 0:
                out[2 * i] = (3 * s[i] + s[i - 1] + 8) >> 4
            if i < n - 1:
                out[2 * i + 1] = (3 * s[i] + s[i + 1] + 7) >> 4
    return out.astype(np.uint8)


def upsample(c, width, height, hs, vs):
    """The chroma plane c (whole MCUs) -> [height, width]; only its first ceil(H/vs) rows and ceil(W/hs) columns contribute."""
    if hs == 1 and vs == 1:
        return c[:height, :width]
    assert hs == 2
    n, m = (width + 1) // 2, (height + vs - 1) // vs
    c = c[:m, :n]
    out = np.zeros((height, 2 * n), np.uint8)
    for y in range(height):
        if vs == 1:
            out[y] = upsample_row(c[y])
        elif n <= 2:
            out[y] = upsample_row(c[y // 2])
        else:
            r = y // 2
            nb = max(r - 1, 0) if y % 2 == 0 else min(r + 1, m - 1)
            out[y] = upsample_row(c[r], c[nb])
    return out[:, :width]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(coef, qts, width, height, ncomp, hs, vs):
    """The picture P of a flagged descriptor: coef in the download layout, qts[c] the 64 quantisers of component c (natural order)."""
    grids = unit_grids(coef, width, height, ncomp, hs, vs)
    planes = [plane_from_units(idct_units(g, np.asarray(qts[c]).reshape(64))) for c, g in enumerate(grids)]
    yp = planes[0][:height, :width]
    if ncomp == 1:
        return np.stack([yp, yp, yp], axis=-1)
    return ycc_to_rgb(yp, upsample(planes[1], width, height, hs, vs), upsample(planes[2], width, height, hs, vs))
