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

// ---- the reduced transforms of PJD_F_LIBJPEG_SCALE_* (libjpeg jidctred.c, CONST_BITS = 13; normative text: include/pjd.h) ----
// One 1-D pass of jpeg_idct_4x4 before its rounding shift.  i[4] is never read: pass 1 skips column 4, pass 2 column 4 of the workspace.
static inline __host__ __device__ void pjd_lj_idct1d_4(const uint32_t i[8], uint32_t o[4])
{
    const uint32_t t0 = i[0] << 14, t2 = i[2] * 15137u + i[6] * (uint32_t)-6270;
    const uint32_t t10 = t0 + t2, t12 = t0 - t2;
    const uint32_t a0 = i[7] * (uint32_t)-1730 + i[5] * 11893u + i[3] * (uint32_t)-17799 + i[1] * 8697u;
    const uint32_t a2 = i[7] * (uint32_t)-4176 + i[5] * (uint32_t)-4926 + i[3] * 7373u + i[1] * 20995u;
    o[0] = t10 + a2; o[3] = t10 - a2;
    o[1] = t12 + a0; o[2] = t12 - a0;
}
// One 1-D pass of jpeg_idct_2x2: reads i[0], i[1], i[3], i[5], i[7]
static inline __host__ __device__ void pjd_lj_idct1d_2(const uint32_t i[8], uint32_t o[2])
{
    const uint32_t t10 = i[0] << 15;
    const uint32_t t0 = i[7] * (uint32_t)-5906 + i[5] * 6967u + i[3] * (uint32_t)-10426 + i[1] * 29692u;
    o[0] = t10 + t0; o[1] = t10 - t0;
}
// The transform of size M (8, 4, 2): its 1-D kernel, the rounding shifts of its two passes, the columns (pass 2: workspace columns)
// it reads -- COLS of them, the k-th being col(k)
template <int M> struct PjdLjRed;
template <> struct PjdLjRed<8> {
    enum { COLS = 8, SH1 = PJD_LJ_PASS1_SHIFT, SH2 = PJD_LJ_PASS2_SHIFT };
    static inline __host__ __device__ uint32_t col(uint32_t k) { return k; }
    static inline __host__ __device__ void run(const uint32_t i[8], uint32_t o[8]) { pjd_lj_idct1d(i, o); }
};
template <> struct PjdLjRed<4> {
    enum { COLS = 7, SH1 = 12, SH2 = 19 };
    static inline __host__ __device__ uint32_t col(uint32_t k) { return k < 4u ? k : k + 1u; }            // 0 1 2 3 5 6 7
    static inline __host__ __device__ void run(const uint32_t i[8], uint32_t o[4]) { pjd_lj_idct1d_4(i, o); }
};
template <> struct PjdLjRed<2> {
    enum { COLS = 5, SH1 = 13, SH2 = 20 };
    static inline __host__ __device__ uint32_t col(uint32_t k) { return k < 2u ? k : 2u * k - 1u; }       // 0 1 3 5 7
    static inline __host__ __device__ void run(const uint32_t i[8], uint32_t o[2]) { pjd_lj_idct1d_2(i, o); }
};
template <int S>
static inline __host__ __device__ uint32_t pjd_lj_sample_sh(uint32_t o) { return (uint32_t)pjd_lj_clamp255((int32_t)pjd_lj_descale<S>(o) + 128); }
// jpeg_idct_1x1: the sample of a unit's dequantised DC term
static inline __host__ __device__ uint32_t pjd_lj_sample_1x1(uint32_t d0) { return pjd_lj_sample_sh<3>(d0); }

// One unit through the transform of size M on the host's terms (coef, q natural order; out M x M): what pjd_libjpeg_idct_scaled exports
template <int M>
static inline __host__ __device__ void pjd_lj_idct_unit(const int16_t *coef, const uint16_t *q, uint8_t *out)
{
    typedef PjdLjRed<M> T;
    uint32_t ws[M][8];
    for (uint32_t k = 0; k < (uint32_t)T::COLS; k++) {
        const uint32_t c = T::col(k);
        uint32_t x[8], o[M];
        for (int j = 0; j < 8; j++) x[j] = pjd_lj_dequant((int)coef[j * 8 + c], q[j * 8 + c]);
        T::run(x, o);
        for (int j = 0; j < M; j++) ws[j][c] = pjd_lj_descale<T::SH1>(o[j]);
    }
    for (int r = 0; r < M; r++) {
        uint32_t x[8], o[M];
        for (int j = 0; j < 8; j++) x[j] = 0;
        for (uint32_t k = 0; k < (uint32_t)T::COLS; k++) x[T::col(k)] = ws[r][T::col(k)];
        T::run(x, o);
        for (int j = 0; j < M; j++) out[r * M + j] = (uint8_t)pjd_lj_sample_sh<T::SH2>(o[j]);
    }
}

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
