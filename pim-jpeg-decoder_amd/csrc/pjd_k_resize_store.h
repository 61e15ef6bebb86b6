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

// The colour map of pjd_batch_set_colour (the kernels built with COL; normative in include/pjd.h) on a lane's finished row: every pixel's
// 8-bit triple through the output's 3 x 4 map in Q16 -- per sample three 24-bit multiply-adds (the first takes o + 32768), a shift and
// one med3 (pjd_colour_calc of pjd_internal.h, the code pjd_colour_value exports).  `m` is the record of the tile's OUTPUT: wave-uniform,
// read through the index that picks recs[lo], so it lies in scalar registers and the multiplies take their weights from there.  A
// record flagged PJD_COL_IDENTITY skips the arithmetic under a wave-uniform branch: the same bytes, since the identity is exact.
__device__ __forceinline__ void colour_px(uint32_t (&px)[3][PJD_RS_PX], const PjdDevColour &m)
{
    if (m.flags & PJD_COL_IDENTITY) return;                // uniform
    const int32_t half[3] = {m.o[0] + 32768, m.o[1] + 32768, m.o[2] + 32768};
#pragma unroll
    for (int q = 0; q < PJD_RS_PX; q++) {
        const uint32_t r = px[0][q], g = px[1][q], b = px[2][q];
#pragma unroll
        for (int c = 0; c < 3; c++) px[c][q] = pjd_colour_calc(m.q[c], half[c], r, g, b);
    }
}

// ... and on all finished rows of a tile at once, in place, under ONE such branch (the table-driven body, which holds the whole tile in
// its accumulators: a branch per row there costs a third of the kernel's registers -- 205 VGPRs against 146, profiles/colour_matrix.md)
__device__ __forceinline__ void colour_tile(uint32_t (&px)[PJD_RS_ROWS][3][PJD_RS_PX], const PjdDevColour &m)
{
    if (m.flags & PJD_COL_IDENTITY) return;                // uniform
    const int32_t half[3] = {m.o[0] + 32768, m.o[1] + 32768, m.o[2] + 32768};
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++)
#pragma unroll
        for (int q = 0; q < PJD_RS_PX; q++) {
            const uint32_t r = px[k][0][q], g = px[k][1][q], b = px[k][2][q];
#pragma unroll
            for (int c = 0; c < 3; c++) px[k][c][q] = pjd_colour_calc(m.q[c], half[c], r, g, b);
        }
}

// NC: the channels stored, 3, or 1 only where PLANAR (a grey batch: one plane)
template <bool PLANAR, int DT, int NC = 3>
__device__ __forceinline__ void store_row(const uint32_t (&px)[3][PJD_RS_PX], uint8_t *dp, uint32_t row, uint32_t col0, uint32_t n_px,
                                          uint64_t dst_plane, uint32_t dst_stride, const NormArgs &nz)
{
#include "pjd_k_resize_store_body.h"
}

// The transposed form of the epilogue (pjd_batch_set_orientation, orientations 5..8; the kernels built with ORI): the tile's PJD_RS_ROWS
// rows of Q, px[k][c][q] for row row0 + k (k < n_rows) and column col0 + q (q < n_px; 0: nothing), leave as D's rows col0 + q, which
// are r_th samples long.  They lie row_len samples apart: r_th again, or with a pad (pjd_batch_set_resize_pad) the canvas's width, while
// the mirror keeps counting from r_th, the content's.  A lane's rows of one column are adjacent samples of one row of D -- columns row0 .. row0 + 7, or with
// `mirror` r_th - 1 - row0 downwards, which in ascending order is the same eight samples reversed -- so they leave in ONE store per
// column and channel: 8 bytes planar uint8, 16 (fp16 / bf16) or 2 x 16 (fp32) planar floats, 24 bytes (3 x 8) interleaved RGB8, 3 or
// 6 x 16 interleaved floats; where the tile has all its rows and the address has that store's alignment.  Element stores otherwise (a
// ragged last row tile, an unaligned bound output).  Not transposed through LDS: a tile has eight rows of Q, so no store of D can be
// longer than eight samples whichever lane issues it.
// The eight samples are held in D's order relative to `jv`, the column of the first one if the tile had all its rows (negative for a
// mirrored ragged tile: then only elements are stored, and only those of rows that exist).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool PLANAR, int DT, int NC = 3>
__device__ __forceinline__ void store_cols(const uint32_t (&px)[PJD_RS_ROWS][3][PJD_RS_PX], uint8_t *dp, uint32_t row0, uint32_t n_rows, uint32_t col0,
                                           uint32_t n_px, bool mirror, uint32_t r_th, uint32_t row_len, uint64_t dst_plane, const NormArgs &nz)
{
    constexpr int R = PJD_RS_ROWS;
    static_assert(R == 8, "the packing below is written for eight rows");
    static_assert(NC == 3 || (NC == 1 && PLANAR), "one channel is one plane");
    constexpr uint32_t ES = DT == 0 ? 1u : PJD_DT_SIZE(DT);
    const bool full = n_rows == (uint32_t)R;
    const int64_t jv = mirror ? (int64_t)r_th - (int64_t)row0 - R : (int64_t)row0;
#pragma unroll
    for (int q = 0; q < PJD_RS_PX; q++) {
        if ((uint32_t)q >= n_px) break;
        const int64_t first = (int64_t)((uint64_t)(col0 + q) * row_len) + jv;          // in samples of one channel, from the picture's (plane's) start
        uint32_t v[3][R];                                  // D's order
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int m = 0; m < R; m++) v[c][m] = mirror ? px[R - 1 - m][c][q] : px[m][c][q];
        // element m is row (mirror ? 7 - m : m) of the tile
#define PJD_COL_EXISTS(m) ((mirror ? (uint32_t)(R - 1 - (m)) : (uint32_t)(m)) < n_rows)
        if (PLANAR) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                uint8_t *o = dp + ((int64_t)((uint64_t)c * dst_plane) + first) * (int64_t)ES;
                if (DT == 0) {
                    if (full && ((uintptr_t)o & 7u) == 0) {
                        *reinterpret_cast<u32x2 *>(o) = u32x2{v[c][0] | (v[c][1] << 8) | (v[c][2] << 16) | (v[c][3] << 24),
                                                             v[c][4] | (v[c][5] << 8) | (v[c][6] << 16) | (v[c][7] << 24)};
                    } else {
#pragma unroll
                        for (int m = 0; m < R; m++)
                            if (PJD_COL_EXISTS(m)) o[m] = (uint8_t)v[c][m];
                    }
                } else if (DT == PJD_DT_F32) {
                    float e[R];
#pragma unroll
                    for (int m = 0; m < R; m++) e[m] = pjd_normalize_f32(v[c][m], nz.scale[c], nz.bias[c]);
                    if (full && ((uintptr_t)o & 15u) == 0) {
                        f32x4 *o4 = reinterpret_cast<f32x4 *>(o);
                        o4[0] = f32x4{e[0], e[1], e[2], e[3]};
                        o4[1] = f32x4{e[4], e[5], e[6], e[7]};
                    } else {
#pragma unroll
                        for (int m = 0; m < R; m++)
                            if (PJD_COL_EXISTS(m)) reinterpret_cast<float *>(o)[m] = e[m];
                    }
                } else {
                    uint32_t d[R / 2];
#pragma unroll
                    for (int p = 0; p < R / 2; p++) d[p] = norm_pair16<DT>(v[c][2 * p], v[c][2 * p + 1], nz.scale[c], nz.bias[c]);
                    if (full && ((uintptr_t)o & 15u) == 0) {
                        *reinterpret_cast<u32x4 *>(o) = u32x4{d[0], d[1], d[2], d[3]};
                    } else {
#pragma unroll
                        for (int m = 0; m < R; m++)
                            if (PJD_COL_EXISTS(m)) reinterpret_cast<uint16_t *>(o)[m] = (uint16_t)(d[m >> 1] >> (16 * (m & 1)));
                    }
                }
            }
        } else {
            uint8_t *o = dp + 3 * first * (int64_t)ES;
            if (DT == 0) {
                if (full && ((uintptr_t)o & 7u) == 0) {
                    uint32_t d[3 * R / 4];                 // byte t of the 24 is channel t % 3 of sample t / 3
#pragma unroll
                    for (int p = 0; p < 3 * R / 4; p++)
                        d[p] = v[(4 * p) % 3][(4 * p) / 3] | (v[(4 * p + 1) % 3][(4 * p + 1) / 3] << 8) | (v[(4 * p + 2) % 3][(4 * p + 2) / 3] << 16) |
                               (v[(4 * p + 3) % 3][(4 * p + 3) / 3] << 24);
                    u32x2 *o2 = reinterpret_cast<u32x2 *>(o);
                    o2[0] = u32x2{d[0], d[1]};
                    o2[1] = u32x2{d[2], d[3]};
                    o2[2] = u32x2{d[4], d[5]};
                } else {
#pragma unroll
                    for (int m = 0; m < R; m++)
                        if (PJD_COL_EXISTS(m))
#pragma unroll
                            for (int c = 0; c < 3; c++) o[3 * m + c] = (uint8_t)v[c][m];
                }
            } else if (DT == PJD_DT_F32) {
                float e[3 * R];                            // R0 G0 B0 R1 ...
#pragma unroll
                for (int m = 0; m < R; m++)
#pragma unroll
                    for (int c = 0; c < 3; c++) e[3 * m + c] = pjd_normalize_f32(v[c][m], nz.scale[c], nz.bias[c]);
                if (full && ((uintptr_t)o & 15u) == 0) {
                    f32x4 *o4 = reinterpret_cast<f32x4 *>(o);
#pragma unroll
                    for (int p = 0; p < 3 * R / 4; p++) o4[p] = f32x4{e[4 * p], e[4 * p + 1], e[4 * p + 2], e[4 * p + 3]};
                } else {
#pragma unroll
                    for (int m = 0; m < R; m++)
                        if (PJD_COL_EXISTS(m))
#pragma unroll
                            for (int c = 0; c < 3; c++) reinterpret_cast<float *>(o)[3 * m + c] = e[3 * m + c];
                }
            } else {
                uint32_t h[3 * R];                         // a pair spans two channels, so the elements are made one by one
#pragma unroll
                for (int m = 0; m < R; m++)
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float u = pjd_normalize_f32(v[c][m], nz.scale[c], nz.bias[c]);
                        h[3 * m + c] = DT == PJD_DT_F16 ? (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)u) : (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)u);
                    }
                if (full && ((uintptr_t)o & 15u) == 0) {
                    u32x4 *o4 = reinterpret_cast<u32x4 *>(o);
#pragma unroll
                    for (int p = 0; p < 3 * R / 8; p++)
                        o4[p] = u32x4{h[8 * p] | (h[8 * p + 1] << 16), h[8 * p + 2] | (h[8 * p + 3] << 16), h[8 * p + 4] | (h[8 * p + 5] << 16), h[8 * p + 6] | (h[8 * p + 7] << 16)};
                } else {
#pragma unroll
                    for (int m = 0; m < R; m++)
                        if (PJD_COL_EXISTS(m))
#pragma unroll
                            for (int c = 0; c < 3; c++) reinterpret_cast<uint16_t *>(o)[3 * m + c] = (uint16_t)h[3 * m + c];
                }
            }
        }
#undef PJD_COL_EXISTS
    }
}
