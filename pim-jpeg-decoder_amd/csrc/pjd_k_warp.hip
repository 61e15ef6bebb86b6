// pjd_k_warp.hip -- affine warp on decode (pjd_batch_set_resize_affine): every output of a batch, read from its picture as the back end
// left it at its decode size in the batch's intermediate buffer, under its own inverse 2 x 3 map -- rotation, scale, shear,
// translation -- with the fill where the map looks outside the picture, in ONE launch that writes every byte of every output.  The
// filter is the bilinear one include/pjd.h specifies bit for bit, in 64-bit fixed point (Q40); its taps come from pjd_warp_pos and
// pjd_warp_fix (pjd_internal.h), the functions pjd_warp_tap exports.
//
// A gather that no axis table can serve: the map is not separable.  One wave takes one tile of one output (pjd_k_warp_body.h says
// which shape and why), a lane PJD_RS_PX adjacent pixels of each of its rows, and the rows leave through the epilogue of the resample
// (store_row of pjd_k_resize_store.h, called as it is): uint8 or normalised fp16 / bf16 / fp32 elements, planar or interleaved, vector
// stores where the address has their alignment.  The source is read with byte loads; neighbouring lanes' taps fall into the same or
// adjacent cache lines whatever the angle.  No LDS, no scratch.
//
// Twelve kernels: interleaved and planar x (uint8, fp16, bf16, fp32) with three channels, and the one-plane form of a grey batch;
// eight more with a colour map (pjd_k_warp_col).
// Wave-uniform values -- the record of the output, the fill, the six constants of a normalised launch -- come through readfirstlane
// and the kernel arguments.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

#include "pjd_k_resize_store.h"

template <bool PLANAR, int DT, int NC>
__global__ void __launch_bounds__(64 * PJD_WARP_WAVES)
pjd_k_warp(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs, const PjdDevWarp *__restrict__ warp,
           const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, uint32_t fill, const NormArgs nz)
{
    static_assert(NC == 3 || (NC == 1 && PLANAR), "one channel is one plane");
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
#include "pjd_k_warp_body.h"
}

// With a colour map (pjd_batch_set_colour): the same body with COL -- colour_px of pjd_k_resize_store.h on every finished row, the
// fill included -- in kernels of their own, so that a batch without one launches exactly what it launched before.  Three channels.
template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_WARP_WAVES)
pjd_k_warp_col(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs, const PjdDevWarp *__restrict__ warp,
               const PjdDevColour *__restrict__ colour, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, uint32_t fill,
               const NormArgs nz)
{
    constexpr bool COL = true;
    constexpr int NC = 3;
#include "pjd_k_warp_body.h"
}

template <bool PLANAR, int NC>
void launch(hipStream_t s, const PjdWarpLaunch &a, const NormArgs &nz)
{
    const dim3 grid((a.n_tiles + PJD_WARP_WAVES - 1) / PJD_WARP_WAVES), block(64 * PJD_WARP_WAVES);
    switch (a.norm.dtype) {
    case 0:           hipLaunchKernelGGL((pjd_k_warp<PLANAR, 0, NC>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    case PJD_DT_F16:  hipLaunchKernelGGL((pjd_k_warp<PLANAR, PJD_DT_F16, NC>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    case PJD_DT_BF16: hipLaunchKernelGGL((pjd_k_warp<PLANAR, PJD_DT_BF16, NC>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    default:          hipLaunchKernelGGL((pjd_k_warp<PLANAR, PJD_DT_F32, NC>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    }
}

template <bool PLANAR>
void launch_col(hipStream_t s, const PjdWarpLaunch &a, const NormArgs &nz)
{
    const dim3 grid((a.n_tiles + PJD_WARP_WAVES - 1) / PJD_WARP_WAVES), block(64 * PJD_WARP_WAVES);
    switch (a.norm.dtype) {
    case 0:           hipLaunchKernelGGL((pjd_k_warp_col<PLANAR, 0>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    case PJD_DT_F16:  hipLaunchKernelGGL((pjd_k_warp_col<PLANAR, PJD_DT_F16>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    case PJD_DT_BF16: hipLaunchKernelGGL((pjd_k_warp_col<PLANAR, PJD_DT_BF16>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    default:          hipLaunchKernelGGL((pjd_k_warp_col<PLANAR, PJD_DT_F32>), grid, block, 0, s, a.src, a.dst, a.recs, a.warp, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.fill, nz); break;
    }
}

}  // namespace

void pjd_launch_warp(hipStream_t s, const PjdWarpLaunch &a)
{
    if (a.n_tiles == 0) return;
    NormArgs nz{};
    for (int c = 0; c < 3; c++) { nz.scale[c] = a.norm.scale[c]; nz.bias[c] = a.norm.bias[c]; }
    if (a.colour) { if (a.planar) launch_col<true>(s, a, nz); else launch_col<false>(s, a, nz); }   // a coloured batch: three channels
    else if (a.channels == 1) launch<true, 1>(s, a, nz);   // a grey batch: planar, one plane
    else if (a.planar) launch<true, 3>(s, a, nz);
    else launch<false, 3>(s, a, nz);
}
