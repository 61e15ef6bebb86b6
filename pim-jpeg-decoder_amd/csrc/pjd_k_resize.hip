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
#include <hip/hip_runtime.h>

#include "pjd_kernels.h"

namespace {

// ((256 - w) * a + w * b): below 2^16; the products and sums of the second stage stay below 2^24 (include/pjd.h)
__device__ __forceinline__ uint32_t lerp8(uint32_t a, uint32_t b, uint32_t w) { return __umul24(256u - w, a) + __umul24(w, b); }

template <bool PLANAR>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
             const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * PJD_RS_WAVES + (threadIdx.x >> 6));
    if (tile >= n_tiles) return;
    // the picture of this tile: the last one whose prefix is <= tile (pictures without tiles do not exist: every target has a pixel)
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    const PjdDevResize r = recs[lo];
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_RS_ROWS;
    const uint32_t col0 = (t % r.col_tiles) * PJD_RS_COLS + lane * PJD_RS_PX;

    // row taps: lane k (k < PJD_RS_ROWS) computes those of row row0 + k, and they are read back as scalars (y0 | wy << 16) here, while
    // every lane is still active
    uint32_t rowtap[PJD_RS_ROWS];
    {
        const uint32_t row = row0 + (lane & (PJD_RS_ROWS - 1));
        uint32_t y0, y1, wy;
        pjd_resize_tap_calc(r.sh, r.th, row < r.th ? row : r.th - 1, y0, y1, wy);
        const uint32_t packed = y0 | (wy << 16);
#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) rowtap[k] = __builtin_amdgcn_readlane(packed, k);
    }
    if (col0 >= r.tw) return;                              // only now: the lanes that computed row taps may have no column

    uint32_t x0[PJD_RS_PX], x1[PJD_RS_PX], wx[PJD_RS_PX];
#pragma unroll
    for (int k = 0; k < PJD_RS_PX; k++) {
        const uint32_t x = col0 + k;
        pjd_resize_tap_calc(r.sw, r.tw, x < r.tw ? x : r.tw - 1, x0[k], x1[k], wx[k]);
        if (!PLANAR) { x0[k] *= 3u; x1[k] *= 3u; }          // byte offsets in an interleaved row
    }
    const uint32_t n_px = r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX;
    const uint8_t *sp = src + r.src_off;
    uint8_t *dp = dst + r.dst_off;
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;        // from one channel to the next
    const uint64_t dst_plane = PLANAR ? (uint64_t)r.tw * r.th : 1u;
    const uint32_t dst_stride = PLANAR ? r.tw : 3u * r.tw;

#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        const uint32_t row = row0 + k;
        if (row >= r.th) break;                            // uniform
        const uint32_t y0 = rowtap[k] & 0xffffu, wy = rowtap[k] >> 16, y1 = y0 + 1u < r.sh ? y0 + 1u : r.sh - 1u;
        const uint8_t *s0 = sp + (uint64_t)y0 * r.src_stride, *s1 = sp + (uint64_t)y1 * r.src_stride;
        uint32_t px[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t *c0 = s0 + c * src_plane, *c1 = s1 + c * src_plane;
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                const uint32_t top = lerp8(c0[x0[q]], c0[x1[q]], wx[q]), bot = lerp8(c1[x0[q]], c1[x1[q]], wx[q]);
                px[c][q] = (__umul24(256u - wy, top) + __umul24(wy, bot) + 32768u) >> 16;
            }
        }
        if (PLANAR) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                uint8_t *o = dp + c * dst_plane + (uint64_t)row * dst_stride + col0;
                if (n_px == PJD_RS_PX && ((uintptr_t)o & 3u) == 0)
                    *reinterpret_cast<uint32_t *>(o) = px[c][0] | (px[c][1] << 8) | (px[c][2] << 16) | (px[c][3] << 24);
                else
                    for (uint32_t q = 0; q < n_px; q++) o[q] = (uint8_t)px[c][q];
            }
        } else {
            uint8_t *o = dp + (uint64_t)row * dst_stride + 3u * col0;
            if (n_px == PJD_RS_PX && ((uintptr_t)o & 3u) == 0) {
                struct alignas(4) U3 { uint32_t a, b, c; } v;
                v.a = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[0][1] << 24);
                v.b = px[1][1] | (px[2][1] << 8) | (px[0][2] << 16) | (px[1][2] << 24);
                v.c = px[2][2] | (px[0][3] << 8) | (px[1][3] << 16) | (px[2][3] << 24);
                *reinterpret_cast<U3 *>(o) = v;
            } else {
                for (uint32_t q = 0; q < n_px; q++)
                    for (int c = 0; c < 3; c++) o[3 * q + c] = (uint8_t)px[c][q];
            }
        }
    }
}

}  // namespace

void pjd_launch_resize(hipStream_t s, const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const uint32_t *tile_prefix, uint32_t n_images,
                       uint32_t n_tiles, bool planar)
{
    if (n_tiles == 0) return;
    const dim3 grid((n_tiles + PJD_RS_WAVES - 1) / PJD_RS_WAVES), block(64 * PJD_RS_WAVES);
    if (planar) hipLaunchKernelGGL(pjd_k_resize<true>, grid, block, 0, s, src, dst, recs, tile_prefix, n_images, n_tiles);
    else hipLaunchKernelGGL(pjd_k_resize<false>, grid, block, 0, s, src, dst, recs, tile_prefix, n_images, n_tiles);
}
