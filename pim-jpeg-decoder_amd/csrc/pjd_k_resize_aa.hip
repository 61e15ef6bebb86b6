// pjd_k_resize_aa.hip -- the antialiased resize on decode (pjd_batch_set_resize_filter, PJD_RESIZE_ANTIALIAS): the launch of
// pjd_k_resize.hip with the widened triangle filter include/pjd.h specifies bit for bit.  The work division is that launch's: one
// launch for the ragged batch, the same tiles and prefix sum (PJD_RS_ROWS target rows x PJD_RS_COLS target columns per wave), a lane
// PJD_RS_PX = 4 adjacent pixels of each row of its tile.  A workgroup is ONE wave here: its barriers cost nothing.
//
// An output sample has up to 32 x 32 taps, so nothing is gathered.  The filter is separable; a wave STREAMS down the source rows its
// tile reads, and for each of them
//   - stages the row's segment -- the source columns the tile's 256 target columns read -- in LDS with coalesced dword loads (the
//     segment starts wherever it starts: the dword that holds its first byte is the first one loaded, and the taps read behind the
//     remainder `sh`);
//   - filters it horizontally, once per tile and not once per target row: per lane 4 pixels x 3 channels, the taps as byte reads from
//     LDS (neighbouring lanes share most of them), the weights from the batch's table (tap-major: adjacent lanes, adjacent words;
//     padded with weight 0 up to the axis' largest count, so the loop bound is uniform) -> twelve h16;
//   - adds w * h16 to the accumulators of those of the tile's 8 target rows that have this source row among their taps -- a
//     wave-uniform test, the weight a scalar load.  8 x 12 accumulators live in registers (no scratch).
// Then the epilogue of pjd_k_resize_body.h: round, pack or normalise and convert, and store with the same alignment fall-backs.
// No lane leaves before the last barrier; lanes right of the picture compute its last column and store nothing.
//
// The weights are made on the host (pjd_resize_aa_taps_calc, pjd_internal.h) by pjd_batch_set_resize_filter: no division here.
#include <hip/hip_runtime.h>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

#include "pjd_k_resize_store.h"

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_aa(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa,
                const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];                      // one source row's segment (three plane segments where PLANAR)
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles) return;                           // uniform, as everything up to `col0`
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    const PjdDevResize r = recs[lo];
    const PjdDevResizeAA a = aa[lo];
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_RS_ROWS;
    const uint32_t colt = (t % r.col_tiles) * PJD_RS_COLS;
    const uint32_t col0 = colt + lane * PJD_RS_PX;
    const uint32_t *xt = tab + a.x_tab, *yt = tab + a.y_tab;

    // the source columns of the tile: from the first tap of its first column to the last tap of its last one
    const uint32_t col_last = colt + PJD_RS_COLS - 1u < r.tw ? colt + PJD_RS_COLS - 1u : r.tw - 1u;
    const uint32_t head0 = xt[colt], head1 = xt[col_last];
    const uint32_t xs = head0 & 0xffffu, xe = (head1 & 0xffffu) + (head1 >> 16), span = xe - xs;
    const uint32_t pitch = (span + 6u) & ~3u;              // bytes per plane segment (PLANAR)
    if (xe > r.sw || xe <= xs || pjd_resize_aa_lds(span, PLANAR) > lds_bytes) return;   // never with the host's table: nothing is read or written out of bounds

    // the source rows of the tile, and per target row its first tap and tap count
    uint32_t yf[PJD_RS_ROWS], yc[PJD_RS_ROWS];
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        const uint32_t row = row0 + k < r.th ? row0 + k : r.th - 1u;
        const uint32_t head = yt[row];
        yf[k] = head & 0xffffu;
        yc[k] = row0 + k < r.th ? head >> 16 : 0u;         // rows below the picture take nothing
    }
    const uint32_t row_last = row0 + PJD_RS_ROWS - 1u < r.th ? row0 + PJD_RS_ROWS - 1u : r.th - 1u;
    const uint32_t head_l = yt[row_last];
    const uint32_t ys = yf[0], ye_ = (head_l & 0xffffu) + (head_l >> 16), ye = ye_ < r.sh ? ye_ : r.sh;

    // per lane: its four columns (the picture's last one for those right of it) and their first taps, relative to the segment
    uint32_t xcol[PJD_RS_PX], xf[PJD_RS_PX];
#pragma unroll
    for (int q = 0; q < PJD_RS_PX; q++) {
        xcol[q] = col0 + q < r.tw ? col0 + q : r.tw - 1u;
        xf[q] = (xt[xcol[q]] & 0xffffu) - xs;
    }
    const uint32_t n_px = col0 >= r.tw ? 0u : (r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX);
    const uint8_t *sp = src + r.src_off;
    uint8_t *dp = dst + r.dst_off;
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;
    const uint64_t dst_plane = PLANAR ? (uint64_t)r.tw * r.th : 1u;
    const uint32_t dst_stride = PLANAR ? r.tw : 3u * r.tw;
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(seg);

    uint32_t acc[PJD_RS_ROWS][3][PJD_RS_PX];
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++)
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] = 0u;

    for (uint32_t y = ys; y < ye; y++) {
        __syncthreads();                                   // the taps of the row before have been read
        uint32_t sh[3];                                    // bytes between the first dword staged and the segment's first byte
        if (PLANAR) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint8_t *g = sp + c * src_plane + (uint64_t)y * r.src_stride + xs;
                sh[c] = (uint32_t)((uintptr_t)g & 3u);
                const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g - sh[c]);
                const uint32_t nd = (sh[c] + span + 3u) >> 2;
                for (uint32_t d = lane; d < nd; d += 64u) seg[c * (pitch >> 2) + d] = g4[d];
            }
        } else {
            const uint8_t *g = sp + (uint64_t)y * r.src_stride + 3u * xs;
            sh[0] = (uint32_t)((uintptr_t)g & 3u);
            const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g - sh[0]);
            const uint32_t nd = (sh[0] + 3u * span + 3u) >> 2;
            for (uint32_t d = lane; d < nd; d += 64u) seg[d] = g4[d];
        }
        __syncthreads();

        uint32_t h[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) h[c][q] = 0u;
        for (uint32_t tp = 0; tp < a.x_taps; tp++) {
            const uint32_t *wrow = xt + (size_t)(tp + 1u) * r.tw;
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                const uint32_t w = wrow[xcol[q]];
                const uint32_t j = xf[q] + tp < span ? xf[q] + tp : span - 1u;    // past the column's count the weight is 0: any staged byte
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const uint32_t v = PLANAR ? sb[c * pitch + sh[c] + j] : sb[sh[0] + 3u * j + c];
                    h[c][q] += __umul24(w, v);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) h[c][q] = (h[c][q] + 128u) >> 8;

#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) {
            const uint32_t d = y - yf[k];                  // wraps where the row's taps start below y
            if (d < yc[k]) {                               // uniform
                const uint32_t w = yt[(size_t)(d + 1u) * r.th + row0 + k];
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] += __umul24(w, h[c][q]);
            }
        }
    }

#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        if (row0 + k >= r.th) break;                       // uniform
        uint32_t px[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) px[c][q] = (acc[k][c][q] + (1u << 23)) >> 24;
        store_row<PLANAR, DT>(px, dp, row0 + k, col0, n_px, dst_plane, dst_stride, nz);
    }
}

}  // namespace

void pjd_launch_resize_aa(hipStream_t s, const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const uint32_t *tile_prefix, uint32_t n_images,
                          uint32_t n_tiles, bool planar, const PjdNormalize &norm, const PjdDevResizeAA *aa, const uint32_t *tab, uint32_t lds_bytes)
{
    if (n_tiles == 0) return;
    const dim3 grid(n_tiles), block(64);
    NormArgs nz{};
    for (int c = 0; c < 3; c++) { nz.scale[c] = norm.scale[c]; nz.bias[c] = norm.bias[c]; }
#define PJD_RS_AA(P, D) hipLaunchKernelGGL((pjd_k_resize_aa<P, D>), grid, block, lds_bytes, s, src, dst, recs, tile_prefix, n_images, n_tiles, aa, tab, lds_bytes, nz)
    switch (norm.dtype) {
    case 0:           if (planar) PJD_RS_AA(true, 0);           else PJD_RS_AA(false, 0);           break;
    case PJD_DT_F16:  if (planar) PJD_RS_AA(true, PJD_DT_F16);  else PJD_RS_AA(false, PJD_DT_F16);  break;
    case PJD_DT_BF16: if (planar) PJD_RS_AA(true, PJD_DT_BF16); else PJD_RS_AA(false, PJD_DT_BF16); break;
    default:          if (planar) PJD_RS_AA(true, PJD_DT_F32);  else PJD_RS_AA(false, PJD_DT_F32);  break;
    }
#undef PJD_RS_AA
}
