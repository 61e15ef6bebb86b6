// pjd_k_resize_win.hip -- resize on decode with source windows (pjd_batch_set_resize_window): the two resample launches of
// pjd_k_resize.hip and pjd_k_resize_aa.hip for a batch whose pictures are resampled from a WINDOW of the decoded picture to a window
// of a virtual target, mirrored left-right where asked -- flip(resize(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]) of include/pjd.h.
// No arithmetic of its own: the taps are pjd_resize_tap_calc (bilinear) and the host's weight table (antialiased) with a shifted
// index.  The tile grid, the prefix sum, the lanes' four pixels and the stores are those of the un-windowed launches, so that
// everything pjd_batch_set_resize promises (one launch named "resize", every byte of every range and none outside, any alignment of a
// bound destination) holds word for word.  A batch without windows never comes here: it runs the kernels it ran before.
// The per-picture window is a record of its own (PjdDevResizeWin) beside PjdDevResize, whose layout the other units keep.
#include <hip/hip_runtime.h>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

#include "pjd_k_resize_store.h"

// ((256 - w) * a + w * b): below 2^16 (pjd_k_resize.hip)
__device__ __forceinline__ uint32_t lerp8(uint32_t a, uint32_t b, uint32_t w) { return __umul24(256u - w, a) + __umul24(w, b); }

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_win(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                 const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                 const NormArgs nz)
{
#include "pjd_k_resize_win_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_win_aa(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                    const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                    const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];                      // one source row's segment (three plane segments where PLANAR)
#include "pjd_k_resize_win_aa_body.h"
}

}  // namespace

void pjd_launch_resize_win(hipStream_t s, const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const PjdDevResizeWin *win,
                           const uint32_t *tile_prefix, uint32_t n_images, uint32_t n_tiles, bool planar, const PjdNormalize &norm, bool antialias,
                           const PjdDevResizeAA *aa, const uint32_t *tab, uint32_t lds_bytes)
{
    if (n_tiles == 0) return;
    NormArgs nz{};
    for (int c = 0; c < 3; c++) { nz.scale[c] = norm.scale[c]; nz.bias[c] = norm.bias[c]; }
    if (antialias) {
        const dim3 grid(n_tiles), block(64);
#define PJD_RS_WIN(P, D) hipLaunchKernelGGL((pjd_k_resize_win_aa<P, D>), grid, block, lds_bytes, s, src, dst, recs, win, tile_prefix, n_images, n_tiles, aa, tab, lds_bytes, nz)
        switch (norm.dtype) {
        case 0:           if (planar) PJD_RS_WIN(true, 0);           else PJD_RS_WIN(false, 0);           break;
        case PJD_DT_F16:  if (planar) PJD_RS_WIN(true, PJD_DT_F16);  else PJD_RS_WIN(false, PJD_DT_F16);  break;
        case PJD_DT_BF16: if (planar) PJD_RS_WIN(true, PJD_DT_BF16); else PJD_RS_WIN(false, PJD_DT_BF16); break;
        default:          if (planar) PJD_RS_WIN(true, PJD_DT_F32);  else PJD_RS_WIN(false, PJD_DT_F32);  break;
        }
#undef PJD_RS_WIN
        return;
    }
    const dim3 grid((n_tiles + PJD_RS_WAVES - 1) / PJD_RS_WAVES), block(64 * PJD_RS_WAVES);
#define PJD_RS_WIN(P, D) hipLaunchKernelGGL((pjd_k_resize_win<P, D>), grid, block, 0, s, src, dst, recs, win, tile_prefix, n_images, n_tiles, nz)
    switch (norm.dtype) {
    case 0:           if (planar) PJD_RS_WIN(true, 0);           else PJD_RS_WIN(false, 0);           break;
    case PJD_DT_F16:  if (planar) PJD_RS_WIN(true, PJD_DT_F16);  else PJD_RS_WIN(false, PJD_DT_F16);  break;
    case PJD_DT_BF16: if (planar) PJD_RS_WIN(true, PJD_DT_BF16); else PJD_RS_WIN(false, PJD_DT_BF16); break;
    default:          if (planar) PJD_RS_WIN(true, PJD_DT_F32);  else PJD_RS_WIN(false, PJD_DT_F32);  break;
    }
#undef PJD_RS_WIN
}
