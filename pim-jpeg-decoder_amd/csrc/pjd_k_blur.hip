// pjd_k_blur.hip -- Gaussian blur on decode (pjd_batch_set_blur): every output of a batch, read as the uint8 picture U that the resample
// (or warp) launch of a blurred batch left in the batch's blur intermediate, through the separable filter include/pjd.h specifies bit
// for bit -- its own taps from the host's table, the reflect border, the triangle filter's unsigned arithmetic -- into its final range,
// in ONE launch that writes every byte of every output.  Outputs without a blur pass through as a copy, normalised and laid out here.
//
// A neighbourhood filter: every sample reads ksize x ksize samples around it, across the resample's tiles, so it cannot ride in the
// resample's epilogue as the colour map does.  One workgroup takes one tile of one output (pjd_k_blur_body.h says how: staged bytes
// with their halo, the row pass once per staged row into 16-bit samples, the column pass in registers), one channel at a time, so that
// the dynamic LDS -- sized by the batch's largest radius, pjd_blur_lds -- stays at 17.4 KiB for 23 taps and 29.5 KiB for 63, and the rows
// leave through the epilogue of the resample (store_row of pjd_k_resize_store.h, called as it is).  No scratch.
//
// Twelve kernels: interleaved and planar x (uint8, fp16, bf16, fp32) with three channels, and the one-plane form of a grey batch.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

#include "pjd_k_resize_store.h"

template <bool PLANAR, int DT, int NC>
__global__ void __launch_bounds__(PJD_BLUR_THREADS)
pjd_k_blur(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevBlur *__restrict__ recs, const uint32_t *__restrict__ tile_prefix,
           const uint32_t *__restrict__ taps, uint32_t n_images, uint32_t n_tiles, uint32_t lds_bytes, const NormArgs nz)
{
    static_assert(NC == 3 || (NC == 1 && PLANAR), "one channel is one plane");
    extern __shared__ uint32_t lds[];
#include "pjd_k_blur_body.h"
}

template <bool PLANAR, int NC>
void launch(hipStream_t s, const PjdBlurLaunch &a, const NormArgs &nz)
{
    const dim3 grid(a.n_tiles), block(PJD_BLUR_THREADS);
    switch (a.norm.dtype) {
    case 0:           hipLaunchKernelGGL((pjd_k_blur<PLANAR, 0, NC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.taps, a.n_images, a.n_tiles, a.lds_bytes, nz); break;
    case PJD_DT_F16:  hipLaunchKernelGGL((pjd_k_blur<PLANAR, PJD_DT_F16, NC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.taps, a.n_images, a.n_tiles, a.lds_bytes, nz); break;
    case PJD_DT_BF16: hipLaunchKernelGGL((pjd_k_blur<PLANAR, PJD_DT_BF16, NC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.taps, a.n_images, a.n_tiles, a.lds_bytes, nz); break;
    default:          hipLaunchKernelGGL((pjd_k_blur<PLANAR, PJD_DT_F32, NC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.taps, a.n_images, a.n_tiles, a.lds_bytes, nz); break;
    }
}

}  // namespace

void pjd_launch_blur(hipStream_t s, const PjdBlurLaunch &a)
{
    if (a.n_tiles == 0) return;
    NormArgs nz{};
    for (int c = 0; c < 3; c++) { nz.scale[c] = a.norm.scale[c]; nz.bias[c] = a.norm.bias[c]; }
    if (a.channels == 1) launch<true, 1>(s, a, nz);        // a grey batch: planar, one plane
    else if (a.planar) launch<true, 3>(s, a, nz);
    else launch<false, 3>(s, a, nz);
}
