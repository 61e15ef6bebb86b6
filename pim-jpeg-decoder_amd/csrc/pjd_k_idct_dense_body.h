// pjd_k_idct_dense_body.h -- the body of the dense colour kernels, included once per kernel by pjd_k_backend.hip:
// pjd_k_idct_colour<SCALED> with PJD_DENSE_PLANAR = false, pjd_k_idct_colour_planar<SCALED> with PJD_DENSE_PLANAR = true.
// One text for both, and textual inclusion rather than a shared function on purpose: with the body moved into a function,
// pjd_k_idct_colour<false> took three more registers (39 -> 42); included, it compiles to the instructions it had when it stood in
// the kernel (profiles/planar_output.md).  Uses the kernel's parameters B, wgs, dense_base and its template parameter SCALED.
// What a lane does with the 16 bytes it loads is pjd_k_dense_stage_body.h, which pjd_k_idct_gray<SCALED> includes too.
#ifndef PJD_DENSE_PLANAR
#error "define PJD_DENSE_PLANAR (false / true) before including pjd_k_idct_dense_body.h"
#endif
    __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
    __shared__ uint16_t qs[3][64];
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];

    const PjdDevIdctWg wg = wgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t tid = threadIdx.x;
    const uint32_t dus = im.dus_per_mcu, nl = im.n_luma;
    const uint32_t n_du = wg.n_mcu * dus;
    const uint32_t RI = im.restart_interval;

    if (tid < 192) qs[tid >> 6][tid & 63] = B.qtab[(size_t)wg.image * 192 + tid];
    __syncthreads();

    // ---- load (16 B per lane, coalesced), de-zigzag, dequantise: lane (du, r) owns zigzag slots 8r..8r+7 on load; after the scatter
    // to natural order pjd_tile_to_pixels does the passes
    const int16_t *cbase = B.coef + (dense_base[wg.pad_] + (uint64_t)(wg.first_mcu - im.first_mcu) * dus) * 64;
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) {
        const uint32_t du = i >> 3, r = i & 7;
        const uint32_t ml = du / dus, k = du - ml * dus;
        const uint32_t comp = k < nl ? 0 : k - nl + 1;
        const int4 raw = *reinterpret_cast<const int4 *>(cbase + (size_t)du * 64 + r * 8);
#define PJD_DENSE_Q qs[comp]
#include "pjd_k_dense_stage_body.h"
#undef PJD_DENSE_Q
    }
    __syncthreads();
    pjd_tile_to_pixels<true, SCALED, PJD_DENSE_PLANAR>(tile, mcu_xy, B, im, wg, tid);
