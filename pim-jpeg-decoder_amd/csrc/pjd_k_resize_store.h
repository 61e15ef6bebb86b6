// pjd_k_resize_store.h -- what the resample kernels of pjd_k_resize.hip share beside their bodies: the launch constants, the native
// vectors, the blend and the epilogue as a function.  Included inside the unit's anonymous namespace, behind <hip/hip_runtime.h>,
// include/pjd.h and pjd_kernels.h (tools/resize_host.cpp includes it the same way).

// ((256 - w) * a + w * b): below 2^16; the products and sums of the second stage stay below 2^24 (include/pjd.h)
__device__ __forceinline__ uint32_t lerp8(uint32_t a, uint32_t b, uint32_t w) { return __umul24(256u - w, a) + __umul24(w, b); }

// The arithmetic of the two table-driven filters (pjd_k_resize_aa_body.h; normative in include/pjd.h), FILT a compile-time constant.
// The triangle filter: weights 0..65536, everything unsigned, the row sample with 8 fraction bits.  The bicubic filter: weights of
// either sign (|q| < 2^18) held as the bit patterns of int32, sums in two's complement, the row sample with 6 fraction bits
// (|h6| < 2^15) and ONE clamp, at the end (v_med3_i32).  Every product has operands of at most 24 signed bits.
template <int FILT>
__device__ __forceinline__ uint32_t tap_mac(uint32_t acc, uint32_t w, uint32_t v)
{
    if (FILT == PJD_RESIZE_BICUBIC) return acc + (uint32_t)__mul24((int32_t)w, (int32_t)v);
    return acc + __umul24(w, v);
}
template <int FILT>
__device__ __forceinline__ uint32_t tap_row(uint32_t h)
{
    if (FILT == PJD_RESIZE_BICUBIC) return (uint32_t)(((int32_t)h + 512) >> 10);
    return (h + 128u) >> 8;
}
template <int FILT>
__device__ __forceinline__ uint32_t tap_out(uint32_t v)
{
    if (FILT == PJD_RESIZE_BICUBIC) {
        const int32_t o = ((int32_t)v + (1 << 21)) >> 22;
        return (uint32_t)(o < 0 ? 0 : o > 255 ? 255 : o);
    }
    return (v + (1u << 23)) >> 24;
}

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

template <bool PLANAR, int DT>
__device__ __forceinline__ void store_row(const uint32_t (&px)[3][PJD_RS_PX], uint8_t *dp, uint32_t row, uint32_t col0, uint32_t n_px,
                                          uint64_t dst_plane, uint32_t dst_stride, const NormArgs &nz)
{
#include "pjd_k_resize_store_body.h"
}
