// pjd_k_backend_std.hip -- the back end of PJD_F_LIBJPEG pictures (include/pjd.h: islow IDCT, fancy upsampling, JFIF colour).
//
// Two launches, because fancy upsampling reads the chroma of neighbouring MCUs and a back-end range is a run of at most
// PJD_IDCT_MAX_DU units of one MCU row or several:
//   pjd_k_idct_std_lanes / pjd_k_idct_std_dense
//                       the front ends of pjd_k_backend.hip -- the group parser of the lane streams (the same text, included), the
//                       dense scratch of the exact kernel -- staging the coefficients AS DECODED (int16), then jpeg_idct_islow:
//                       pass 1 multiplies by the quantiser in 32 bits and runs on columns into a 32-bit LDS workspace, pass 2 runs
//                       on its rows and stores 8 samples of a component PLANE (uint8, padded to whole MCUs) as one 8-byte store
//   pjd_k_colour_std    upsample + colour + store: a thread makes four adjacent pixels of one row and writes them where the
//                       default back end writes them -- RGB8, planar or the BMP image
// Each of the three has a _red twin for the pictures with PJD_F_LIBJPEG_SCALE_* (libjpeg's reduced IDCTs, planes of the reduced geometry).
// What a kernel shares with its twin is written once: the lane-stream front end is pjd_std_lanes<RED>, the dense front end
// pjd_k_libjpeg_dense_body.h (one text for these two kernels and the grey unit's two), the plane geometry pjd_std_planes at (n, cn), the
// colour kernels' tail pjd_std_store4; a pair differs in its passes (pjd_std_idct_to_planes / pjd_std_red_to_planes) and, for the colour
// kernels, in the picture's size and the chroma fetch.
// The arithmetic is pjd_libjpeg.h's, which the host entry points export; the two passes over the LDS tile are pjd_libjpeg_passes.h's, the
// dense staging pjd_k_dense_stage_body.h's and the walk over the luma units pjd_k_backend_common.h's, all shared with the grey unit.
// pjd_launch_idct_std_lanes / _std_dense launch these kernels or, for a grey batch, the grey unit's, through one helper for the two-part
// lists (full size, then reduced).
#include "pjd_libjpeg_passes.h"

namespace {

struct PjdStdPlanes {
    uint8_t *p[3];
    uint32_t stride[3];
};

// The planes of a picture whose luma units are n and whose chroma units are cn samples a side (8, 8 at full size): whole MCUs, luma
// mcux*hs*n x mcuy*vs*n, then Cb and Cr of mcux*cn x mcuy*cn each
__device__ __forceinline__ PjdStdPlanes pjd_std_planes(uint8_t *planes, const PjdDevImage &im, uint32_t n, uint32_t cn)
{
    PjdStdPlanes P;
    const uint32_t yw = im.mcux * im.hs * n, yh = im.mcuy * im.vs * n, cw = im.mcux * cn, ch = im.mcuy * cn;
    P.p[0] = planes + (size_t)im.plane_off256 * 256;
    P.p[1] = P.p[0] + (size_t)yw * yh;
    P.p[2] = P.p[1] + (size_t)cw * ch;
    P.stride[0] = yw; P.stride[1] = cw; P.stride[2] = cw;
    return P;
}

// Both passes and the plane store for the n_du units staged in `tile` (natural order, as decoded); mcu_xy holds the grid position
// of the range's MCUs.  Ends with the units' samples in the planes; no barrier behind the stores.
__device__ __forceinline__ void pjd_std_idct_to_planes(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t (*qn)[64],
                                                       const uint32_t *mcu_xy, const PjdDevImage &im, uint32_t n_du, uint8_t *planes, uint32_t tid)
{
    const uint32_t dus = im.dus_per_mcu, nl = im.n_luma, hs = im.hs;
    // pass 1: a thread takes one column of one unit
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) {
        const uint32_t u = i >> 3, c = i & 7;
        const uint32_t ml = pjd_div_small(u, c_recip16[dus]), kk = u - __umul24(ml, dus);
        const uint16_t *q = qn[kk < nl ? 0 : kk - nl + 1];
        PJD_LJ_PASS1_COL(tile, ws, u, q, c);
    }
    __syncthreads();
    // pass 2: a thread takes one row of one unit and stores its 8 samples
    const PjdStdPlanes P = pjd_std_planes(planes, im, 8, 8);
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) {
        const uint32_t u = i >> 3, r = i & 7;
        const uint32_t ml = pjd_div_small(u, c_recip16[dus]), kk = u - __umul24(ml, dus);
        const uint32_t xy = mcu_xy[ml], mx = xy & 0xffffu, my = xy >> 16;
        uint32_t comp, ux, uy;
        if (kk < nl) { comp = 0; ux = mx * hs + (kk & (hs - 1)); uy = my * im.vs + (kk >> (hs - 1)); }
        else { comp = kk - nl + 1; ux = mx; uy = my; }
        // planes are whole MCUs wide and high: every unit of the picture lies inside, 8-byte aligned
        *reinterpret_cast<uint2 *>(P.p[comp] + (size_t)(uy * 8 + r) * P.stride[comp] + ux * 8) = pjd_lj_pass2_row(ws, u, r);
    }
}

// =============================================================================================
// PJD_F_LIBJPEG_SCALE_*: the flagged pictures libjpeg decodes through its reduced IDCTs (include/pjd.h), in the _red kernels.  A luma unit
// becomes N x N samples, N = 4, 2 or 1, a chroma unit CN x CN, CN = N or, for 4:2:0, 2N (pjd_lj_chroma_size), through PjdLjRed<M> of
// pjd_libjpeg.h, and the planes have that geometry (pjd_std_planes).  (N, CN) is a property of the PICTURE, so of the workgroup: one uniform
// switch picks the instantiation, and inside it the luma units and the chroma units of the range are walked in loops of their own, each
// with its size at compile time -- no lane chooses a transform.
// =============================================================================================
// unit j of one class of a range's units -- the luma units (j counts them alone, MCU after MCU), or the chroma units (two per MCU) -- ->
// its MCU of the range, its index among all units of the range, its component and its position in that component's grid of units
template <bool CHROMA>
__device__ __forceinline__ void pjd_std_red_unit(uint32_t j, const PjdDevImage &im, const uint32_t *mcu_xy, uint32_t &u, uint32_t &comp, uint32_t &ux, uint32_t &uy)
{
    const uint32_t nl = im.n_luma, hs = im.hs, dus = im.dus_per_mcu;
    if (CHROMA) {
        const uint32_t ml = j >> 1, xy = mcu_xy[ml];
        comp = 1u + (j & 1u); u = __umul24(ml, dus) + nl + (j & 1u); ux = xy & 0xffffu; uy = xy >> 16;
    } else {
        const PjdLumaUnits L = pjd_luma_units(dus, nl);
        const uint2 at = pjd_luma_unit_xy(j, L, hs, im.vs, mcu_xy, 1u);
        comp = 0; u = pjd_luma_unit(j, L); ux = at.x; uy = at.y;
    }
}

// pass 1 of the n_units units of one class at size M: a thread takes one of the COLS columns the transform reads of one unit.  M = 8 is the
// full pass (the chroma of a 4:2:0 picture at 1/2); M = 1 has no pass 1.
template <int M, bool CHROMA>
__device__ __forceinline__ void pjd_std_red_pass1(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t (*qn)[64], const uint32_t *mcu_xy,
                                                  const PjdDevImage &im, uint32_t n_units, uint32_t tid)
{
    if (M == 1) return;
    constexpr uint32_t COLS = M == 8 ? 8 : (M == 4 ? 7 : 5);
    for (uint32_t i = tid; i < n_units * COLS; i += PJD_IDCT_THREADS) {
        const uint32_t j = COLS == 8 ? i >> 3 : pjd_div_small(i, c_recip16[COLS]), k = i - j * COLS;      // i < 8 * PJD_IDCT_MAX_DU: exact
        uint32_t u, comp, ux, uy;
        pjd_std_red_unit<CHROMA>(j, im, mcu_xy, u, comp, ux, uy);
        const uint16_t *q = qn[comp];
        if (M == 8) PJD_LJ_PASS1_COL(tile, ws, u, q, k);
        else pjd_lj_red_pass1_col<(M == 2 ? 2 : 4)>(tile, ws, u, q, k);
    }
}

// pass 2 and the plane store: a thread takes one of the M rows of one unit and stores its M samples as one store (planes are whole MCUs:
// a row of a unit starts at a multiple of M bytes of a plane whose size is a multiple of 4 wherever M > 1)
template <int M, bool CHROMA>
__device__ __forceinline__ void pjd_std_red_pass2(const int16_t (*tile)[TILE_STRIDE], const uint32_t (*ws)[WS_STRIDE], const uint16_t (*qn)[64], const uint32_t *mcu_xy,
                                                  const PjdDevImage &im, uint32_t n_units, const PjdStdPlanes &P, uint32_t tid)
{
    constexpr uint32_t M_LOG = M == 8 ? 3 : (M == 4 ? 2 : (M == 2 ? 1 : 0));
    for (uint32_t i = tid; i < (n_units << M_LOG); i += PJD_IDCT_THREADS) {
        const uint32_t j = i >> M_LOG, r = i & (M - 1u);
        uint32_t u, comp, ux, uy;
        pjd_std_red_unit<CHROMA>(j, im, mcu_xy, u, comp, ux, uy);
        // the plane by a select, not by an index: an indexed PjdStdPlanes lives in scratch memory
        uint8_t *plane = CHROMA ? (comp == 1u ? P.p[1] : P.p[2]) : P.p[0];
        uint8_t *dst = plane + (size_t)(uy * M + r) * (CHROMA ? P.stride[1] : P.stride[0]) + ux * M;
        if (M == 8) *reinterpret_cast<uint2 *>(dst) = pjd_lj_pass2_row(ws, u, r);
        else if (M == 4) *reinterpret_cast<uint32_t *>(dst) = pjd_lj_red_pass2_row<4>(ws, u, r);
        else if (M == 2) *reinterpret_cast<uint16_t *>(dst) = (uint16_t)pjd_lj_red_pass2_row<2>(ws, u, r);
        else *dst = (uint8_t)pjd_lj_sample_1x1(pjd_lj_dequant((int)tile[u][0], qn[comp][0]));
    }
}

template <int N, int CN>
__device__ __forceinline__ void pjd_std_red_body(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t (*qn)[64], const uint32_t *mcu_xy,
                                                 const PjdDevImage &im, uint32_t n_mcu, uint8_t *planes, uint32_t tid)
{
    const uint32_t n_lu = n_mcu * im.n_luma, n_cu = im.ncomp == 3 ? n_mcu * 2u : 0u;
    pjd_std_red_pass1<N, false>(tile, ws, qn, mcu_xy, im, n_lu, tid);
    pjd_std_red_pass1<CN, true>(tile, ws, qn, mcu_xy, im, n_cu, tid);
    __syncthreads();
    const PjdStdPlanes P = pjd_std_planes(planes, im, N, CN);
    pjd_std_red_pass2<N, false>(tile, ws, qn, mcu_xy, im, n_lu, P, tid);
    pjd_std_red_pass2<CN, true>(tile, ws, qn, mcu_xy, im, n_cu, P, tid);
}

// the picture's (N, CN): uniform over the workgroup
__device__ __forceinline__ void pjd_std_red_to_planes(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t (*qn)[64], const uint32_t *mcu_xy,
                                                      const PjdDevImage &im, uint32_t n_mcu, uint8_t *planes, uint32_t tid)
{
    const uint32_t sl = (im.flags & PJD_IF_LJSCALE_MASK) >> PJD_IF_LJSCALE_SHIFT;
    const bool dbl = im.hs == 2 && im.vs == 2;                  // pjd_lj_chroma_size: 4:2:0 alone doubles
    switch (sl) {
        case 1: if (dbl) pjd_std_red_body<4, 8>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); else pjd_std_red_body<4, 4>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); break;
        case 2: if (dbl) pjd_std_red_body<2, 4>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); else pjd_std_red_body<2, 2>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); break;
        case 3: if (dbl) pjd_std_red_body<1, 2>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); else pjd_std_red_body<1, 1>(tile, ws, qn, mcu_xy, im, n_mcu, planes, tid); break;
        default: break;                                         // never: the planner sends full-size pictures to the kernels above
    }
}

// ---------------------------------------------------------------------------------------------
// The two front ends, each the body of a full-size kernel and of its _red kernel (RED), which differ in the passes behind the staging.
// Lane streams: one workgroup = one back-end range, as in pjd_k_idct_colour_lanes.  order: the launch's workgroup -> index into
// PjdDevBatch::iwgs / marks (the ranges of the flagged pictures).
// ---------------------------------------------------------------------------------------------
template <bool RED>
__device__ __forceinline__ void pjd_std_lanes(const PjdDevBatch &B, const uint32_t *order, uint8_t *planes)
{
    PJD_LANES_LDS_TILE
    __shared__ __attribute__((aligned(16))) uint32_t ws[PJD_IDCT_MAX_DU][WS_STRIDE];
    __shared__ uint16_t qn[3][64];            // per component: the quantiser by natural position
    PJD_LANES_LDS_TABLES                      // qz here: 1 | natural position << 16 (the parser stores what was decoded)

    const uint32_t iwg = order[blockIdx.x];
    if (threadIdx.x < 192) qn[threadIdx.x >> 6][threadIdx.x & 63] = B.qtab[(size_t)B.iwgs[iwg].image * 192 + threadIdx.x];
#define PJD_LANES_RAW
#include "pjd_k_lanes_parse_body.h"
#undef PJD_LANES_RAW
    if (wv == 0) {
#include "pjd_k_lanes_dc_body.h"
    }
    __syncthreads();
    if (RED) pjd_std_red_to_planes(tile, ws, qn, mcu_xy, im, wg.n_mcu, planes, tid);
    else pjd_std_idct_to_planes(tile, ws, qn, mcu_xy, im, n_du, planes, tid);
}

// The tail of the two colour kernels, colour + store of one item: the luma samples yv (first pixel in the low byte) and the chroma samples
// cb, cr of the four adjacent pixels from column X of row y of a width x height picture -> the pixels, where the batch's form puts them;
// pixels past the right edge are not stored.
__device__ __forceinline__ void pjd_std_store4(uint8_t *out, uint32_t flags, uint32_t ncomp, uint32_t width, uint32_t height, uint32_t stride, uint32_t y, uint32_t X,
                                               uint32_t yv, const int (&cb)[4], const int (&cr)[4])
{
    const bool bmp = (flags & PJD_IF_BMP) != 0;
    uint32_t f[4], g[4], l[4];            // first / middle / last byte of a pixel: R, G, B -- B, G, R in the BMP image
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int r_, g_, b_;
        const int yy = (int)((yv >> (8 * k)) & 255);
        if (ncomp < 3) r_ = g_ = b_ = yy;
        else pjd_lj_ycc_to_rgb(yy, cb[k], cr[k], r_, g_, b_);
        f[k] = (uint32_t)(bmp ? b_ : r_); g[k] = (uint32_t)g_; l[k] = (uint32_t)(bmp ? r_ : b_);
    }
    const uint32_t left = width - X;      // pixels of the item that belong to the picture: 1..4 count
    if (flags & PJD_IF_PLANAR) {
        const size_t plane = (size_t)stride * height;
        uint8_t *o = out + (size_t)y * stride + X;
        if (left >= 4) {
            reinterpret_cast<PjdPx4 *>(o)->a = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
            reinterpret_cast<PjdPx4 *>(o + plane)->a = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
            reinterpret_cast<PjdPx4 *>(o + 2 * plane)->a = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
        } else {
            for (uint32_t k = 0; k < left; k++) { o[k] = (uint8_t)f[k]; o[plane + k] = (uint8_t)g[k]; o[2 * plane + k] = (uint8_t)l[k]; }
        }
        return;
    }
    uint8_t *o = bmp ? out + 26 + (size_t)(height - 1 - y) * stride + X * 3 : out + (size_t)y * stride + X * 3;
    if (left >= 4) {
        PjdPx12 v;
        v.a = f[0] | (g[0] << 8) | (l[0] << 16) | (f[1] << 24);
        v.b = g[1] | (l[1] << 8) | (f[2] << 16) | (g[2] << 24);
        v.c = l[2] | (f[3] << 8) | (g[3] << 16) | (l[3] << 24);
        *reinterpret_cast<PjdPx12 *>(o) = v;
    } else {
        for (uint32_t k = 0; k < left; k++) { o[3 * k] = (uint8_t)f[k]; o[3 * k + 1] = (uint8_t)g[k]; o[3 * k + 2] = (uint8_t)l[k]; }
    }
}

}  // namespace

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_lanes(PjdDevBatch B, const uint32_t *__restrict__ order, uint8_t *__restrict__ planes)
{
    pjd_std_lanes<false>(B, order, planes);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_lanes_red(PjdDevBatch B, const uint32_t *__restrict__ order, uint8_t *__restrict__ planes)
{
    pjd_std_lanes<true>(B, order, planes);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_dense(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base,
                                                                         uint8_t *__restrict__ planes)
{
#include "pjd_k_libjpeg_dense_body.h"
    pjd_std_idct_to_planes(tile, ws, qn, mcu_xy, im, n_du, planes, tid);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_dense_red(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base,
                                                                             uint8_t *__restrict__ planes)
{
#include "pjd_k_libjpeg_dense_body.h"
    pjd_std_red_to_planes(tile, ws, qn, mcu_xy, im, wg.n_mcu, planes, tid);
}

// ---------------------------------------------------------------------------------------------
// Upsample + colour + store.  cwgs[k] = {image, first item, -, -}: an item is four adjacent pixels of one picture row, items run
// row by row, a workgroup takes PJD_IDCT_THREADS consecutive items of one picture.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_colour_std(PjdDevBatch B, const PjdDevIdctWg *__restrict__ cwgs, uint8_t *__restrict__ planes)
{
    const PjdDevIdctWg wg = cwgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t width = im.width, height = im.height, stride = im.out_stride, flags = im.flags;
    const uint32_t per_row = (width + 3) >> 2;
    const uint32_t item = wg.first_mcu + threadIdx.x;
    uint8_t *out = B.out + im.out_off;
    const bool bmp = (flags & PJD_IF_BMP) != 0;
    if (bmp && wg.first_mcu == 0) pjd_bmp_header(out, width, height, stride, threadIdx.x);
    const uint32_t y = item / per_row, X = (item - y * per_row) * 4;
    if (y >= height) return;
    const PjdStdPlanes P = pjd_std_planes(planes, im, 8, 8);
    const uint32_t yv = *reinterpret_cast<const uint32_t *>(P.p[0] + (size_t)y * P.stride[0] + X);      // X + 3 lies inside the padded plane
    int cb[4], cr[4];
    if (im.ncomp < 3) { cb[0] = cb[1] = cb[2] = cb[3] = 128; cr[0] = cr[1] = cr[2] = cr[3] = 128; }
    else if (im.hs == 1) {
        const size_t o = (size_t)y * P.stride[1] + X;
        const uint32_t bw = *reinterpret_cast<const uint32_t *>(P.p[1] + o), rw = *reinterpret_cast<const uint32_t *>(P.p[2] + o);
#pragma unroll
        for (int k = 0; k < 4; k++) { cb[k] = (bw >> (8 * k)) & 255; cr[k] = (rw >> (8 * k)) & 255; }
    } else {
        // n, m: the samples of the chroma plane that belong to the picture (libjpeg's downsampled_width / _height); what the padded
        // MCUs hold beyond them never contributes
        const uint32_t n = (width + 1) >> 1, cw = P.stride[1];
        size_t row, nb = 0;
        bool v2 = im.vs == 2;
        if (v2) {
            const uint32_t m = (height + 1) >> 1, r = y >> 1;
            const uint32_t rn = (y & 1) ? (r + 1 < m ? r + 1 : m - 1) : (r ? r - 1 : 0);
            row = (size_t)r * cw; nb = (size_t)rn * cw;
        } else row = (size_t)y * cw;
        pjd_lj_upsample4(P.p[1] + row, v2 ? P.p[1] + nb : nullptr, n, X, cb);
        pjd_lj_upsample4(P.p[2] + row, v2 ? P.p[2] + nb : nullptr, n, X, cr);
    }
    pjd_std_store4(out, flags, im.ncomp, width, height, stride, y, X, yv, cb, cr);
}

// ---------------------------------------------------------------------------------------------
// Upsample + colour + store of a reduced picture: pjd_k_colour_std's items and stores over ceil(W/s) x ceil(H/s) and the reduced planes.
// 4:4:4 and 4:2:0 (chroma at 2N) read their chroma sample for sample; 4:2:2 keeps the h2v1 rule -- fancy where N > 1 and the chroma row
// has more than two samples of the picture, replicated otherwise (libjpeg has no fancy upsampling at min_DCT_scaled_size 1).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_colour_std_red(PjdDevBatch B, const PjdDevIdctWg *__restrict__ cwgs, uint8_t *__restrict__ planes)
{
    const PjdDevIdctWg wg = cwgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t flags = im.flags, sl = (flags & PJD_IF_LJSCALE_MASK) >> PJD_IF_LJSCALE_SHIFT, rnd = (1u << sl) - 1u;
    const uint32_t width = (im.width + rnd) >> sl, height = (im.height + rnd) >> sl, stride = im.out_stride;
    const uint32_t per_row = (width + 3) >> 2;
    const uint32_t item = wg.first_mcu + threadIdx.x;
    uint8_t *out = B.out + im.out_off;
    const bool bmp = (flags & PJD_IF_BMP) != 0;
    if (bmp && wg.first_mcu == 0) pjd_bmp_header(out, width, height, stride, threadIdx.x);
    const uint32_t y = item / per_row, X = (item - y * per_row) * 4;
    if (y >= height) return;
    const uint32_t N = 8u >> sl;
    const PjdStdPlanes P = pjd_std_planes(planes, im, N, pjd_lj_chroma_size(N, im.hs, im.vs));
    // a plane row need not be a multiple of 4 bytes: any address (PjdPx4); what lies behind the row's samples is never used (`left`)
    const uint32_t yv = reinterpret_cast<const PjdPx4 *>(P.p[0] + (size_t)y * P.stride[0] + X)->a;
    int cb[4], cr[4];
    if (im.ncomp < 3) { cb[0] = cb[1] = cb[2] = cb[3] = 128; cr[0] = cr[1] = cr[2] = cr[3] = 128; }
    else if (im.hs == 1 || im.vs == 2) {
        const size_t o = (size_t)y * P.stride[1] + X;
        const uint32_t bw = reinterpret_cast<const PjdPx4 *>(P.p[1] + o)->a, rw = reinterpret_cast<const PjdPx4 *>(P.p[2] + o)->a;
#pragma unroll
        for (int k = 0; k < 4; k++) { cb[k] = (bw >> (8 * k)) & 255; cr[k] = (rw >> (8 * k)) & 255; }
    } else {
        // h2v1.  dw: the samples of a chroma row that belong to the picture, ceil(W * N / 16) = ceil(width / 2)
        const uint32_t dw = (width + 1) >> 1;
        const size_t row = (size_t)y * P.stride[1];
        if (N > 1) {                                            // pjd_lj_upsample4 replicates where dw <= 2
            pjd_lj_upsample4(P.p[1] + row, nullptr, dw, X, cb);
            pjd_lj_upsample4(P.p[2] + row, nullptr, dw, X, cr);
        } else {
            const uint32_t i0 = X >> 1, i1 = i0 + 1 < dw ? i0 + 1 : dw - 1;
            cb[0] = cb[1] = P.p[1][row + i0]; cb[2] = cb[3] = P.p[1][row + i1];
            cr[0] = cr[1] = P.p[2][row + i0]; cr[2] = cr[3] = P.p[2][row + i1];
        }
    }
    pjd_std_store4(out, flags, im.ncomp, width, height, stride, y, X, yv, cb, cr);
}

// The launchers take a list in two parts: n_wg ranges (items) of full-size flagged pictures for `full`, then n_red of reduced ones for `red`.
template <typename List, typename... Rest>
static void pjd_launch_two_parts(hipStream_t s, void (*full)(PjdDevBatch, List, Rest...), void (*red)(PjdDevBatch, List, Rest...), const PjdDevBatch &b, List list,
                                 uint32_t n_wg, uint32_t n_red, Rest... rest)
{
    if (n_wg) hipLaunchKernelGGL(full, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, list, rest...);
    if (n_red) hipLaunchKernelGGL(red, dim3(n_red), dim3(PJD_IDCT_THREADS), 0, s, b, list + n_wg, rest...);
}

void pjd_launch_idct_std_lanes(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const uint32_t *order, uint32_t n_wg, uint32_t n_red, uint8_t *planes)
{
    if (f.gray()) pjd_launch_two_parts(s, pjd_gray_lanes_kernel(PJD_GRAY_LIBJPEG), pjd_gray_lanes_kernel(PJD_GRAY_LIBJPEG_RED), b, order, n_wg, n_red);
    else pjd_launch_two_parts(s, pjd_k_idct_std_lanes, pjd_k_idct_std_lanes_red, b, order, n_wg, n_red, planes);
}

void pjd_launch_idct_std_dense(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const PjdDevIdctWg *wgs, const uint64_t *dense_base, uint32_t n_wg, uint32_t n_red,
                               uint8_t *planes)
{
    if (f.gray()) pjd_launch_two_parts(s, pjd_gray_dense_kernel(PJD_GRAY_LIBJPEG), pjd_gray_dense_kernel(PJD_GRAY_LIBJPEG_RED), b, wgs, n_wg, n_red, dense_base);
    else pjd_launch_two_parts(s, pjd_k_idct_std_dense, pjd_k_idct_std_dense_red, b, wgs, n_wg, n_red, dense_base, planes);
}

void pjd_launch_colour_std(hipStream_t s, const PjdDevBatch &b, const PjdDevIdctWg *cwgs, uint32_t n_wg, uint32_t n_red, uint8_t *planes)
{
    pjd_launch_two_parts(s, pjd_k_colour_std, pjd_k_colour_std_red, b, cwgs, n_wg, n_red, planes);
}
