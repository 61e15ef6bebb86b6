// pjd_libjpeg_passes.h -- the two passes of jpeg_idct_islow (pjd_libjpeg.h) as the PJD_F_LIBJPEG back-end kernels run them over the
// LDS tile: pass 1 on the columns of a unit into a 32-bit workspace, pass 2 on its rows into eight samples.  pjd_std_idct_to_planes
// (pjd_k_backend_std.hip) and pjd_gray_std_idct (pjd_k_backend_gray.hip) keep only their walk over the units and their store.
#pragma once
#include "pjd_k_backend_common.h"
#include "pjd_libjpeg.h"

#define WS_STRIDE 72     // int32 per data unit of the pass-1 workspace: 64 + 8 pad.  A ds_write_b32 banks by (a / 4) % 32 within each
                         // half of the wave: its 4 units x 8 columns start 8 banks apart and cover the 32 banks once

// pass 1, column c of unit u of the tile (natural order, as decoded) into the unit's workspace row; q: its quantiser by natural
// position.  A macro: as a function it moved instructions in all four kernels (profiles/backend_shared_stages.md).
#define PJD_LJ_PASS1_COL(tile, ws, u, q, c)                                                                             \
    do {                                                                                                                \
        uint32_t x_[8], o_[8];                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 8; j++) x_[j] = pjd_lj_dequant((int)tile[u][j * 8 + c], q[j * 8 + c]);    \
        pjd_lj_idct1d(x_, o_);                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 8; j++) ws[u][j * 8 + c] = pjd_lj_descale<PJD_LJ_PASS1_SHIFT>(o_[j]);     \
    } while (0)

// ---- the reduced transforms (PJD_F_LIBJPEG_SCALE_*; PjdLjRed<M> of pjd_libjpeg.h), M = 4 or 2 samples a side ----
// pass 1, the k-th column the transform reads (k < COLS: 7 or 5 -- a thread per column READ, none for the skipped ones) of unit u into
// rows 0 .. M-1 of the unit's workspace; the rows the 1-D kernel never reads are not loaded
template <int M>
__device__ __forceinline__ void pjd_lj_red_pass1_col(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], uint32_t u, const uint16_t *q, uint32_t k)
{
    typedef PjdLjRed<M> T;
    const uint32_t c = T::col(k);
    uint32_t x[8], o[M];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = (M == 4 ? j != 4 : (j < 2 || (j & 1))) ? pjd_lj_dequant((int)tile[u][j * 8 + c], q[j * 8 + c]) : 0u;
    T::run(x, o);
#pragma unroll
    for (int j = 0; j < M; j++) ws[u][j * 8 + c] = pjd_lj_descale<T::SH1>(o[j]);
}

// pass 2, row r (< M) of unit u -> the row's M samples, first sample in the low byte.  Workspace columns pass 1 skipped are read (two
// 16-byte reads, as at full size) and never used.
template <int M>
__device__ __forceinline__ uint32_t pjd_lj_red_pass2_row(const uint32_t (*ws)[WS_STRIDE], uint32_t u, uint32_t r)
{
    typedef PjdLjRed<M> T;
    const uint4 lo = *reinterpret_cast<const uint4 *>(&ws[u][r * 8]), hi = *reinterpret_cast<const uint4 *>(&ws[u][r * 8 + 4]);
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t o[M], px = 0;
    T::run(x, o);
#pragma unroll
    for (int j = 0; j < M; j++) px |= pjd_lj_sample_sh<T::SH2>(o[j]) << (8 * j);
    return px;
}

// pass 2, row r of unit u: two 16-byte reads of its workspace row -> the row's eight samples, first sample in the low byte of .x
__device__ __forceinline__ uint2 pjd_lj_pass2_row(const uint32_t (*ws)[WS_STRIDE], uint32_t u, uint32_t r)
{
    const uint4 lo = *reinterpret_cast<const uint4 *>(&ws[u][r * 8]), hi = *reinterpret_cast<const uint4 *>(&ws[u][r * 8 + 4]);
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t o[8];
    pjd_lj_idct1d(x, o);
    uint2 px;
    px.x = pjd_lj_sample(o[0]) | (pjd_lj_sample(o[1]) << 8) | (pjd_lj_sample(o[2]) << 16) | (pjd_lj_sample(o[3]) << 24);
    px.y = pjd_lj_sample(o[4]) | (pjd_lj_sample(o[5]) << 8) | (pjd_lj_sample(o[6]) << 16) | (pjd_lj_sample(o[7]) << 24);
    return px;
}
