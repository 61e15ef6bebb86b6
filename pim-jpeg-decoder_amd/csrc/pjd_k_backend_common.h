// pjd_k_backend_common.h -- what the back-end units (pjd_k_backend.hip, pjd_k_backend_std.hip, pjd_k_backend_gray.hip) share: the LDS tile row, the
// LDS block of a lane-stream kernel, the range of decoded units, the grid positions of a range's MCUs, the walk over a range's luma units, the 1-D IDCT passes over the tile, the wide stores, the BMP header, the wave scans of the DC stage and the tile store of
// the entry parser.  Each of these stands here once; the kernels differ in which units they walk and where they store.
#pragma once
#include "pjd_device_common.h"
#include "pjd_kernels.h"

#define TILE_STRIDE 72   // int16 per data unit in LDS: 64 + 8 pad (144 B = 36 banks)

// The grey unit's kernels, for the launchers of the forms (pjd_kernels.h), which stand in the other two units
typedef void (*PjdLanesKernel)(PjdDevBatch, const uint32_t *);
typedef void (*PjdDenseKernel)(PjdDevBatch, const PjdDevIdctWg *, const uint64_t *);
enum PjdGrayKernel { PJD_GRAY_SCALED = 0, PJD_GRAY_FULL = 1, PJD_GRAY_LIBJPEG = 2, PJD_GRAY_LIBJPEG_RED = 3 };
PjdLanesKernel pjd_gray_lanes_kernel(PjdGrayKernel which);
PjdDenseKernel pjd_gray_dense_kernel(PjdGrayKernel which);

// The LDS of a kernel that parses the lane streams (pjd_k_lanes_parse_body.h, pjd_k_lanes_dc_body.h), declared by all seven of them in
// this order -- LDS offsets are part of a kernel's text.  The PJD_F_LIBJPEG kernels declare ws and qn between the tile and the rest.
#define PJD_LANES_LDS_TILE __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
#define PJD_LANES_LDS_TABLES                                                                                                         \
    __shared__ uint32_t qz[3][64];            /* per component, by zigzag SLOT: quantiser of its natural position | position << 16 */  \
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];                                                                                     \
    __shared__ uint8_t comp_of[PJD_IDCT_MAX_DU];                                                                                     \
    __shared__ uint8_t du_head[PJD_IDCT_MAX_DU];                                                                                     \
    __shared__ uint32_t wagg[2];              /* group parser: groups in the lane window; whether the lane behind it may belong */     \
    __shared__ uint32_t ltab[96];             /* group parser: the window's lane table */
#define PJD_LANES_LDS PJD_LANES_LDS_TILE PJD_LANES_LDS_TABLES

// Data units of a range [first_du, first_du + n_du) the back end materialises: all of them, or those up to the picture's first
// entropy-coding error (the unit that holds it included, unless the error is in its DC symbol: pjd_internal.h, PjdDevImState).
__device__ __forceinline__ uint32_t pjd_units_decoded(unsigned long long err_key, uint32_t first_du, uint32_t n_du)
{
    if (err_key == ~0ull) return n_du;
    const uint32_t stop = (uint32_t)((err_key >> 4) & 0x0fffffffu) + ((err_key & 1u) ? 0u : 1u);
    return stop <= first_du ? 0u : (stop - first_du < n_du ? stop - first_du : n_du);
}

// Grid position (row << 16 | column) of each MCU of a range, by its first threads: the only divisions of a dense kernel
__device__ __forceinline__ void pjd_fill_mcu_xy(uint32_t *mcu_xy, const PjdDevIdctWg &wg, const PjdDevImage &im, uint32_t tid)
{
    if (tid < wg.n_mcu) {
        const uint32_t m = wg.first_mcu + tid, my = m / im.mcux;
        mcu_xy[tid] = (my << 16) | (m - my * im.mcux);
    }
}

// The luma units of a range, counted alone, MCU after MCU: unit j is luma unit j & (nl-1) of the range's MCU j >> nl_log (an MCU holds
// nl = hs * vs = 1, 2 or 4 of them, row by row, in front of its chroma units).  The figures of the walk, made once in front of the loops:
struct PjdLumaUnits { uint32_t dus, nl, nl_log; };
__device__ __forceinline__ PjdLumaUnits pjd_luma_units(uint32_t dus, uint32_t nl)
{
    PjdLumaUnits L;
    L.dus = dus; L.nl = nl; L.nl_log = nl == 4u ? 2u : nl - 1u;
    return L;
}
__device__ __forceinline__ PjdLumaUnits pjd_luma_units(const PjdDevImage &im) { return pjd_luma_units(im.dus_per_mcu, im.n_luma); }
// luma unit j -> its index among all units of the range
__device__ __forceinline__ uint32_t pjd_luma_unit(uint32_t j, const PjdLumaUnits L) { return __umul24(j >> L.nl_log, L.dus) + (j & (L.nl - 1u)); }
// luma unit j -> the position (.x, .y) of its first sample in the luma plane, a unit being m samples a side (8, or 4, 2, 1 behind a
// reduced IDCT; 1: its position in the grid of units); hs, vs: the picture's; mcu_xy: pjd_fill_mcu_xy's, or the parser's
__device__ __forceinline__ uint2 pjd_luma_unit_xy(uint32_t j, const PjdLumaUnits L, uint32_t hs, uint32_t vs, const uint32_t *mcu_xy, uint32_t m)
{
    const uint32_t ml = j >> L.nl_log, k = j & (L.nl - 1u), xy = mcu_xy[ml];
    return make_uint2((__umul24(xy & 0xffffu, hs) + (k & (hs - 1u))) * m, (__umul24(xy >> 16, vs) + (k >> (hs - 1u))) * m);
}

// ---- the 1-D passes of the reference's IDCT on one row / one column of a unit of the tile (reference src/decoder_dpu.c:218-320)
__device__ __forceinline__ void pjd_tile_row(int16_t (*tile)[TILE_STRIDE], uint32_t du, uint32_t r)
{
    int4 raw = *reinterpret_cast<const int4 *>(&tile[du][r * 8]);
    int16_t *rv = reinterpret_cast<int16_t *>(&raw);
    int o[8];
    pjd_idct8(rv[0], rv[1], rv[2], rv[3], rv[4], rv[5], rv[6], rv[7], o);
#pragma unroll
    for (int j = 0; j < 8; j++) rv[j] = (int16_t)o[j];
    *reinterpret_cast<int4 *>(&tile[du][r * 8]) = raw;
}

__device__ __forceinline__ void pjd_tile_col(int16_t (*tile)[TILE_STRIDE], uint32_t du, uint32_t c)
{
    int x[8], o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = tile[du][j * 8 + c];
    pjd_idct8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], o);
#pragma unroll
    for (int j = 0; j < 8; j++) tile[du][j * 8 + c] = (int16_t)o[j];
}

// One dword whatever its address: gfx950 global stores need no alignment (planar pictures start at any byte the caller binds)
struct __attribute__((packed)) PjdPx4 { uint32_t a; };
struct __attribute__((packed)) PjdPx12 { uint32_t a, b, c; };

// BMP file header exactly as reference src/bmp_writer.cpp:32-41
__device__ __forceinline__ void pjd_bmp_header(uint8_t *out, uint32_t width, uint32_t height, uint32_t stride, uint32_t tid)
{
    if (tid >= 26) return;
    const uint32_t size = 26 + height * stride;
    uint8_t hb = 0;
    switch (tid) {
        case 0: hb = 'B'; break;  case 1: hb = 'M'; break;
        case 2: hb = size & 255; break; case 3: hb = (size >> 8) & 255; break;
        case 4: hb = (size >> 16) & 255; break; case 5: hb = (size >> 24) & 255; break;
        case 10: hb = 0x1A; break; case 14: hb = 12; break;
        case 18: hb = width & 255; break; case 19: hb = (width >> 8) & 255; break;
        case 20: hb = height & 255; break; case 21: hb = (height >> 8) & 255; break;
        case 22: hb = 1; break; case 24: hb = 24; break;
        default: hb = 0;
    }
    out[tid] = hb;
}

// Inclusive scans over the 64 lanes of a wave with DPP moves (VALU only, no LDS round trips): shifts inside each row of
// 16 lanes, then the last lane of a row broadcast into the following rows.  Values are unsigned; 0 is the identity of both.
#define PJD_DPP_STEP(OP, v, ctrl, rmask)                                                               \
    do { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rmask, 0xf, false); v = OP(v, t_); } while (0)
__device__ __forceinline__ uint32_t pjd_op_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t pjd_op_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t pjd_op_pkadd(uint32_t a, uint32_t b)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pjd_op_pksub(uint32_t a, uint32_t b)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b)));
}
#define PJD_WAVE_SCAN(OP, v)                                                                           \
    do {                                                                                                \
        PJD_DPP_STEP(OP, v, 0x111, 0xf); PJD_DPP_STEP(OP, v, 0x112, 0xf); PJD_DPP_STEP(OP, v, 0x114, 0xf);  \
        PJD_DPP_STEP(OP, v, 0x118, 0xf); PJD_DPP_STEP(OP, v, 0x142, 0xa); PJD_DPP_STEP(OP, v, 0x143, 0xc);  \
    } while (0)
// the inclusive value of the lane before (0 in lane 0)
__device__ __forceinline__ uint32_t pjd_wave_prev(uint32_t v)
{
    const uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    return r;
}

// tile[u][pos] = v (low 16 bits), the row offset by one full-rate multiply-add
__device__ __forceinline__ void pjd_tile_put(uint32_t tile_lds, uint32_t u, uint32_t pos, uint32_t v)
{
    const uint32_t a = pjd_mad_u24(u, TILE_STRIDE * 2u, tile_lds + 2u * pos);
    *reinterpret_cast<__attribute__((address_space(3))) int16_t *>(a) = (int16_t)v;
}
