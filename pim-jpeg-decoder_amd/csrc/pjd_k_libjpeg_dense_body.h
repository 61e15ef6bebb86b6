// pjd_k_libjpeg_dense_body.h -- the dense front end of the PJD_F_LIBJPEG kernels (pictures of the exact kernel and progressive frames),
// included as the first text of pjd_k_idct_std_dense[_red] (pjd_k_backend_std.hip) and, with PJD_LJ_LUMA_ONLY defined, of
// pjd_k_idct_gray_std_dense[_red] (pjd_k_backend_gray.hip); the kernels differ in the passes they call behind it.  Textual inclusion for
// the reason pjd_k_idct_dense_body.h gives: as a function this text cost every one of the four an instruction, and pjd_k_idct_std_dense_red
// two registers (profiles/backend_shared_stages.md).  Uses the kernel's parameters B, wgs (wgs[k].pad_ = index into dense_base[], as in
// pjd_k_idct_colour) and dense_base.  Leaves behind the LDS arrays tile (the range's units -- with PJD_LJ_LUMA_ONLY its luma units alone --
// in natural order, as decoded: pjd_k_dense_stage_body.h with PJD_DENSE_RAW), ws, qn (the quantisers by natural position: [3][64], or the
// luma row [64]) and mcu_xy, the locals wg, im, tid and -- without PJD_LJ_LUMA_ONLY -- n_du (all units of the range), and a barrier passed.
    __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
    __shared__ __attribute__((aligned(16))) uint32_t ws[PJD_IDCT_MAX_DU][WS_STRIDE];
#ifdef PJD_LJ_LUMA_ONLY
    __shared__ uint16_t qn[64];
#else
    __shared__ uint16_t qn[3][64];
#endif
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];

    const PjdDevIdctWg wg = wgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t tid = threadIdx.x;
#ifdef PJD_LJ_LUMA_ONLY
    const PjdLumaUnits L = pjd_luma_units(im);
    const uint32_t dus = L.dus, n_staged = wg.n_mcu * L.nl;
    if (tid < 64) qn[tid] = B.qtab[(size_t)wg.image * 192 + tid];
#else
    const uint32_t dus = im.dus_per_mcu;
    const uint32_t n_du = wg.n_mcu * dus, n_staged = n_du;
    if (tid < 192) qn[tid >> 6][tid & 63] = B.qtab[(size_t)wg.image * 192 + tid];
#endif
    pjd_fill_mcu_xy(mcu_xy, wg, im, tid);
    const int16_t *cbase = B.coef + (dense_base[wg.pad_] + (uint64_t)(wg.first_mcu - im.first_mcu) * dus) * 64;
    const bool sentinel = !(im.flags & PJD_IF_PROGRESSIVE);
    for (uint32_t i = tid; i < n_staged * 8; i += PJD_IDCT_THREADS) {
#ifdef PJD_LJ_LUMA_ONLY
        const uint32_t du = pjd_luma_unit(i >> 3, L), r = i & 7;
#else
        const uint32_t du = i >> 3, r = i & 7;
#endif
        const int4 raw = *reinterpret_cast<const int4 *>(cbase + (size_t)du * 64 + r * 8);
#define PJD_DENSE_RAW
#include "pjd_k_dense_stage_body.h"
#undef PJD_DENSE_RAW
    }
    __syncthreads();
