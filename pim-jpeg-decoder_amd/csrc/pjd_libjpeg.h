// pjd_libjpeg.h -- the arithmetic of PJD_F_LIBJPEG (normative text: include/pjd.h), host and device.
//
// THE implementation: the kernels of pjd_k_backend_std.hip run these inlines, and pjd_libjpeg_idct / _ycc_to_rgb / _upsample_row
// (pjd_api.hip) export them to the host.  Everything is 32-bit two's complement that wraps: sums and products are written on
// unsigned words (a compiler may assume that signed arithmetic does not overflow), only the rounding shifts are signed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One 1-D pass of jpeg_idct_islow (libjpeg jidctint.c, CONST_BITS = 13) before its rounding shift.
static inline __host__ __device__ void pjd_lj_idct1d(const uint32_t i[8], uint32_t o[8])
{
    uint32_t z1 = (i[2] + i[6]) * 4433u;
    const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
    const uint32_t t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    o[0] = t10 + a3; o[7] = t10 - a3;
    o[1] = t11 + a2; o[6] = t11 - a2;
    o[2] = t12 + a1; o[5] = t12 - a1;
    o[3] = t13 + a0; o[4] = t13 - a0;
}

// (o + (1 << (s - 1))) >> s, arithmetic shift
template <int S>
static inline __host__ __device__ uint32_t pjd_lj_descale(uint32_t o) { return (uint32_t)((int32_t)(o + (1u << (S - 1))) >> S); }
#define PJD_LJ_PASS1_SHIFT 11        // CONST_BITS - PASS1_BITS
#define PJD_LJ_PASS2_SHIFT 18        // CONST_BITS + PASS1_BITS + 3

static inline __host__ __device__ int pjd_lj_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// the sample of a pass-2 output
static inline __host__ __device__ uint32_t pjd_lj_sample(uint32_t o) { return (uint32_t)pjd_lj_clamp255((int32_t)pjd_lj_descale<PJD_LJ_PASS2_SHIFT>(o) + 128); }

// The 32-bit product of a coefficient and its quantiser (|coef| <= 32768, q <= 65535: no overflow)
static inline __host__ __device__ uint32_t pjd_lj_dequant(int coef, uint32_t q) { return (uint32_t)coef * q; }

// ycc_rgb_convert's tables (libjpeg jdcolor.c), 16 fraction bits
static inline __host__ __device__ void pjd_lj_ycc_to_rgb(int y, int cb, int cr, int &r, int &g, int &b)
{
    cb -= 128; cr -= 128;
    r = pjd_lj_clamp255(y + ((91881 * cr + 32768) >> 16));
    g = pjd_lj_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    b = pjd_lj_clamp255(y + ((116130 * cb + 32768) >> 16));
}

// Fancy upsampling (libjpeg jdsample.c), one output sample of chroma sample `cur`: the even output leans on the sample before, the
// odd one on the sample after.  At the ends of a row the neighbour is the sample itself, which is libjpeg's edge rule
// ((4c + 1) >> 2 = (4c + 2) >> 2 = c, and (4s + 8) >> 4, (4s + 7) >> 4 as written there).  h2v2 takes s = 3 * c[row] + c[neighbour row].
static inline __host__ __device__ int pjd_lj_h2v1(int prev, int cur, int next, bool odd) { return odd ? (3 * cur + next + 2) >> 2 : (3 * cur + prev + 1) >> 2; }
static inline __host__ __device__ int pjd_lj_h2v2(int prev, int cur, int next, bool odd) { return odd ? (3 * cur + next + 7) >> 4 : (3 * cur + prev + 8) >> 4; }
// libjpeg switches the fancy routines off for a chroma row of at most two samples: plain replication on both axes
#define PJD_LJ_FANCY_MIN_N 3u

// The four chroma samples under output columns X .. X + 3 (X a multiple of 4) of one output row: `row` is the chroma row the output
// row lies in, `nb` its neighbour row (null: h2v1), n the samples of a chroma row that belong to the picture.
static inline __host__ __device__ void pjd_lj_upsample4(const uint8_t *row, const uint8_t *nb, uint32_t n, uint32_t X, int c[4])
{
    const uint32_t i0 = X >> 1, i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    if (n < PJD_LJ_FANCY_MIN_N) { c[0] = c[1] = row[i0]; c[2] = c[3] = row[i1]; return; }
    const uint32_t ia = i0 ? i0 - 1 : 0, id = i0 + 2 < n ? i0 + 2 : n - 1;
    if (!nb) {
        const int a = row[ia], b = row[i0], e = row[i1], d = row[id];
        c[0] = pjd_lj_h2v1(a, b, e, false); c[1] = pjd_lj_h2v1(a, b, e, true);
        c[2] = pjd_lj_h2v1(b, e, d, false); c[3] = pjd_lj_h2v1(b, e, d, true);
    } else {
        const int a = 3 * row[ia] + nb[ia], b = 3 * row[i0] + nb[i0], e = 3 * row[i1] + nb[i1], d = 3 * row[id] + nb[id];
        c[0] = pjd_lj_h2v2(a, b, e, false); c[1] = pjd_lj_h2v2(a, b, e, true);
        c[2] = pjd_lj_h2v2(b, e, d, false); c[3] = pjd_lj_h2v2(b, e, d, true);
    }
}
