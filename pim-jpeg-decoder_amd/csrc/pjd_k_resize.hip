// pjd_k_resize.hip -- resize on decode (pjd_batch_set_resize): every picture of a ragged batch, as the back end left it at its decode
// size in the batch's intermediate buffer, resampled to its own target size in ONE launch.  The filter is the bilinear one
// include/pjd.h specifies bit for bit; its taps come from pjd_resize_tap_calc (pjd_internal.h), the function pjd_resize_tap exports.
//
// A memory-bound gather.  One wave takes one TILE of one picture (PJD_RS_ROWS target rows x PJD_RS_COLS target columns; the host's
// prefix sum over the pictures' tiles says which), a lane PJD_RS_PX = 4 adjacent pixels of each of its rows:
//   - the column taps (the divisions) are computed once per lane and serve all rows of the tile;
//   - the row taps are computed by the first PJD_RS_ROWS lanes, one row each, and read back as wave-uniform values;
//   - a lane's four pixels leave in one dword store per channel (planar) or three dwords (interleaved) where the address is
//     4-byte aligned and the row has four pixels left -- byte stores at a ragged right edge and for an unaligned destination
//     (pjd_batch_bind_output promises no alignment);
//   - the source is read with byte loads: the gather addresses of neighbouring lanes fall into the same or adjacent cache lines.
// Exactly the bytes of each picture's range are written, every one of them by every launch.
//
// Normalised float output (pjd_batch_set_normalize): the same taps and blends, and where the uint8 variant packs its four samples the
// float variants finish them -- one binary32 fma per sample (pjd_normalize_f32 of pjd_internal.h, the arithmetic include/pjd.h
// specifies), one conversion for the 16-bit types -- and store elements of 2 or 4 bytes: a lane's four pixels of one channel in one
// 8-byte (fp16 / bf16) or 16-byte (fp32) store planar, 24 or 48 bytes interleaved, where the address has that store's alignment and
// the row has four pixels left; element stores otherwise (pjd_batch_bind_output promises element alignment, no more).  The six
// constants are launch arguments: wave-uniform, they never pass through the per-picture record.
#include <hip/hip_runtime.h>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

// ((256 - w) * a + w * b): below 2^16; the products and sums of the second stage stay below 2^24 (include/pjd.h)
__device__ __forceinline__ uint32_t lerp8(uint32_t a, uint32_t b, uint32_t w) { return __umul24(256u - w, a) + __umul24(w, b); }

// the constants of a normalised launch, by value in the kernel arguments (scalar registers)
struct NormArgs { float scale[3], bias[3]; };

// native vectors: one store of the vector's size and alignment (HIP's float4 / uint2 are structs that copy member by member)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two adjacent samples of one channel -> two 16-bit elements in a dword: fma in binary32, then ONE rounding to the 16-bit type
template <int DT>
__device__ __forceinline__ uint32_t norm_pair16(uint32_t v0, uint32_t v1, float scale, float bias)
{
    const f32x2 u = {pjd_normalize_f32(v0, scale, bias), pjd_normalize_f32(v1, scale, bias)};
    if (DT == PJD_DT_F16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(u, f16x2));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(u, bf16x2));
}

template <bool PLANAR>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
             const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles)
{
    constexpr int DT = 0;
    const NormArgs nz{};
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_norm(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                  const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
#include "pjd_k_resize_body.h"
}

}  // namespace

void pjd_launch_resize(hipStream_t s, const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const uint32_t *tile_prefix, uint32_t n_images,
                       uint32_t n_tiles, bool planar, const PjdNormalize &norm)
{
    if (n_tiles == 0) return;
    const dim3 grid((n_tiles + PJD_RS_WAVES - 1) / PJD_RS_WAVES), block(64 * PJD_RS_WAVES);
    if (norm.dtype == 0) {
        if (planar) hipLaunchKernelGGL(pjd_k_resize<true>, grid, block, 0, s, src, dst, recs, tile_prefix, n_images, n_tiles);
        else hipLaunchKernelGGL(pjd_k_resize<false>, grid, block, 0, s, src, dst, recs, tile_prefix, n_images, n_tiles);
        return;
    }
    NormArgs nz;
    for (int c = 0; c < 3; c++) { nz.scale[c] = norm.scale[c]; nz.bias[c] = norm.bias[c]; }
#define PJD_RS_NORM(P, D) hipLaunchKernelGGL((pjd_k_resize_norm<P, D>), grid, block, 0, s, src, dst, recs, tile_prefix, n_images, n_tiles, nz)
    switch (norm.dtype) {
    case PJD_DT_F16:  if (planar) PJD_RS_NORM(true, PJD_DT_F16);  else PJD_RS_NORM(false, PJD_DT_F16);  break;
    case PJD_DT_BF16: if (planar) PJD_RS_NORM(true, PJD_DT_BF16); else PJD_RS_NORM(false, PJD_DT_BF16); break;
    default:          if (planar) PJD_RS_NORM(true, PJD_DT_F32);  else PJD_RS_NORM(false, PJD_DT_F32);  break;
    }
#undef PJD_RS_NORM
}
