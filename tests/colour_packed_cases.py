"""Shared by tests/test_colour_packed_cpu.py and tests/test_gpu_colour_packed.py: a numpy model of the colour stage's packed fast
path (pjd_colour_store, pim-jpeg-decoder_amd/csrc/pjd_k_backend.hip) and pictures whose chroma samples lie on the edges of the
range that sends a task to it.

The fast path needs every chroma term of the conversion, +128 included, in int16, which holds when both chroma samples are in
[-16384, 16383].  A DC coefficient alone cannot bring a sample there: a DC-only block is (int16)(D * 181 >> 9) applied twice, at most
4094 for an int16 D.  So the blocks below hold the DC and eight AC coefficients at the even rows and columns 0, 2, 4 (quantiser 64;
the DC has quantiser 8, so that one step of the DC value moves every sample by about one); their values were found by a search
with the oracle port's IDCT, and test_colour_packed_cpu.py checks with that IDCT that the samples are where they should be."""
import numpy as np

import jpeg_symbols as J
import symbol_corpus as SC

LO, HI = -16384, 16383                       # chroma samples of the fast path

# ---- the model ------------------------------------------------------------------------------------------------------------------
def chroma_terms(cb, cr):
    """The three chroma terms of pjd_ycc_to_rgb, +128 included: (r, g, b) as exact integers."""
    cb, cr = np.asarray(cb, np.int64), np.asarray(cr, np.int64)
    return (5880414 * cr >> 22) + 128, 128 - (1442840 * cb >> 22) - (2994733 * cr >> 22), (7432306 * cb >> 22) + 128


def reference_rgb(y, cb, cr):
    """clamp255(y + term + 128) per channel: the formula of pjd_ycc_to_rgb (reference src/decoder_dpu.c:376-382)."""
    y = np.asarray(y, np.int64)
    return tuple(np.clip(y + t, 0, 255).astype(np.uint8) for t in chroma_terms(cb, cr))


def pk_add_i16_sat(a, b):
    """v_pk_add_i16 ... clamp: per half, the sum of two int16 saturated to int16.  a, b: (..., 2) int16."""
    assert a.dtype == np.int16 and b.dtype == np.int16
    return np.clip(a.astype(np.int32) + b.astype(np.int32), -32768, 32767).astype(np.int16)


def sat_pk_u8_i16(a):
    """v_sat_pk_u8_i16: per half, an int16 saturated to uint8.  a: (..., 2) int16 -> (..., 2) uint8."""
    assert a.dtype == np.int16
    return np.clip(a, 0, 255).astype(np.uint8)


def in_range(*samples):
    """A task takes the fast path only if this holds for every chroma sample under it -- the kernel's test: add 0x4000 to each
    16-bit half modulo 2^16, bit 15 of every half clear."""
    ok = True
    for s in samples:
        h = (np.asarray(s, np.int64).astype(np.uint16).astype(np.uint32) + 0x4000) & 0xffff
        ok = ok & ((h & 0x8000) == 0)
    return ok


def fast_path_rgb(y01, cb01, cr01):
    """One luma pair (y0, y1) with the chroma samples of its two pixels, the way the kernel pairs them: the terms are computed in 32
    bits, truncated to int16 when the pair is packed, added to the packed luma pair with signed saturation, then saturated to bytes.
    Arguments: (..., 2) int16.  Returns (r, g, b), each (..., 2) uint8."""
    out = []
    for t in chroma_terms(cb01, cr01):
        packed = (t & 0xffff).astype(np.uint16).view(np.int16)
        out.append(sat_pk_u8_i16(pk_add_i16_sat(np.asarray(y01, np.int16), packed)))
    return tuple(out)


def div_small(u, d):
    """pjd_div_small(u, c_recip16[d]): (u * ceil(2^16 / d)) >> 16 with a 24-bit multiply."""
    recip = -(-65536 // d)
    return ((u & 0xffffff) * (recip & 0xffffff) & 0xffffffff) >> 16


# ---- the pictures ---------------------------------------------------------------------------------------------------------------
NAT = [0, 2, 4, 16, 18, 20, 32, 34, 36]      # natural positions of a block's nine coefficients
Q_DC, Q_AC = 8, 64
# name -> value of the coefficient at each position of NAT before dequantisation; what the names promise is over the groups of four
# horizontally adjacent samples of the 8 x 8 block:
BLOCKS = {
    "in_max": [-835, 0, 405, 379, -414, 176, -3, -123, 163],       # a group inside [LO, HI] whose maximum is HI
    "out_hi": [-834, 0, 405, 379, -414, 176, -3, -123, 163],       # a group with one sample outside: HI + 1
    "in_min": [233, 363, -396, -205, 32, 0, -424, 268, -113],      # a group inside [LO, HI] whose minimum is LO
    "out_lo": [232, 363, -396, -205, 32, 0, -424, 268, -113],      # a group with one sample outside: LO - 1
    "max": [93] + [412] * 8,                                        # a sample of 32767
    "min": [-93] + [-412] * 8,                                      # a sample of -32768
    "plain": [40, 10, -7, 3, 0, 0, 5, 0, 0],                        # small samples
    "plain2": [-55, 0, 0, -9, 2, 0, 0, 0, 1],
    "zero": [0] * 9,
}
# (Cb, Cr) of consecutive MCUs: in-range and out-of-range chroma in neighbouring MCUs, so that one wave runs both paths
CHROMA = [("in_max", "plain"), ("out_hi", "plain"), ("plain", "in_min"), ("plain2", "out_lo"), ("max", "min"), ("plain", "plain2"),
          ("in_min", "in_max"), ("min", "max"), ("zero", "out_hi"), ("out_lo", "zero"), ("plain2", "plain")]
LUMA = ["plain", "max", "min", "in_max", "zero", "out_lo", "plain2"]
SAMPLINGS = dict(SC.SAMPLINGS, **{"2c": [(1, 1), (1, 1)]})           # "2c": luma and Cb only (the missing Cr reads as 0)


def _tokens(vals, diff, zz_slot):
    """DC difference, then the block's nonzero AC coefficients in zigzag order (with ZRL symbols where a run exceeds 15), then EOB."""
    toks, at = [J.dcv(diff)], 1
    for slot, v in sorted((zz_slot[n], v) for n, v in zip(NAT[1:], vals[1:]) if v):
        run = slot - at
        while run > 15:
            toks.append(J.AC(15, 0))
            run -= 16
        toks.append(J.acv(run, v))
        at = slot + 1
    return toks + [J.EOB]


def frame(w, h, sub, ri=0, std=False):
    comps = [J.Component(hh, vv, min(j, 1), 0, 0) for j, (hh, vv) in enumerate(SAMPLINGS[sub])]
    fr = J.Frame(w, h, comps, {0: SC.dc_general()}, {0: SC.ac_162()}, ri=ri, standard_restart=std)
    zz_slot = {n: k for k, n in enumerate(fr.zigzag()) if k not in (48, 52)}
    for t in {c.tq for c in comps}:
        fr.qt[t] = [1] * 64
        fr.qt[t][0] = Q_DC
        for n in NAT[1:]:
            fr.qt[t][zz_slot[n]] = Q_AC
    return fr, zz_slot


def picture(w, h, sub, ri=0, std=False, first=0):
    """(jpeg, frame, intent, names): MCU m takes CHROMA[(first + m) % len] for its chroma blocks; the luma units cycle through LUMA.
    names[u] is the block of data unit u."""
    fr, zz_slot = frame(w, h, sub, ri, std)
    per = fr.unit_comps()
    names, seen = [], {c: 0 for c in range(len(fr.comps))}
    for u in range(fr.n_units()):
        m, c = u // len(per), per[u % len(per)]
        names.append(LUMA[(first + seen[0]) % len(LUMA)] if c == 0 else CHROMA[(first + m) % len(CHROMA)][c - 1])
        seen[c] += 1
    anchors = {c: [] for c in range(len(fr.comps))}
    k = {c: 0 for c in anchors}
    for u, nm in enumerate(names):
        c = per[u % len(per)]
        anchors[c].append((k[c], BLOCKS[nm][0], "direct"))
        k[c] += 1
    diffs = SC.dc_script(fr, anchors)
    data, it = J.write(fr, [_tokens(BLOCKS[nm], diffs[u], zz_slot) for u, nm in enumerate(names)])
    return data, fr, it, names


def samples_after_idct(port, data, fr, it):
    """The intent's coefficients through the port's dequantisation and IDCT: int16 [n_dpus][25 blocks of 16 x 16][12 units: 4 Y,
    4 Cb, 4 Cr][64]."""
    meta = port.parse(data)["metadata"]
    mcus = J.intent_buffer(fr, it).copy()
    for d in range(mcus.shape[0]):
        port.dpu_stage(meta, mcus[d], 0)
        port.dpu_stage(meta, mcus[d], 1)
    return mcus.reshape(mcus.shape[0], 25, 12, 64)
