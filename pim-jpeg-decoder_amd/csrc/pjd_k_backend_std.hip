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
// The arithmetic is pjd_libjpeg.h's, which the host entry points export; the two passes over the LDS tile are pjd_libjpeg_passes.h's and
// the dense staging pjd_k_dense_stage_body.h's, both shared with the grey unit.  pjd_launch_idct_std_lanes / _std_dense launch these
// kernels or, for a grey batch, the grey unit's.
#include "pjd_libjpeg_passes.h"

namespace {

struct PjdStdPlanes {
    uint8_t *p[3];
    uint32_t stride[3];
};

__device__ __forceinline__ PjdStdPlanes pjd_std_planes(uint8_t *planes, const PjdDevImage &im)
{
    PjdStdPlanes P;
    const uint32_t cw = im.mcux * 8, ch = im.mcuy * 8, yw = cw * im.hs, yh = ch * im.vs;
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
    const PjdStdPlanes P = pjd_std_planes(planes, im);
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

}  // namespace

// ---------------------------------------------------------------------------------------------
// Lane-stream front end: one workgroup = one back-end range, as in pjd_k_idct_colour_lanes.
// order: the launch's workgroup -> index into PjdDevBatch::iwgs / marks (the ranges of the flagged pictures).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_lanes(PjdDevBatch B, const uint32_t *__restrict__ order, uint8_t *__restrict__ planes)
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
    pjd_std_idct_to_planes(tile, ws, qn, mcu_xy, im, n_du, planes, tid);
}

// ---------------------------------------------------------------------------------------------
// Dense front end (pictures of the exact kernel and progressive frames): wgs[k].pad_ = index into dense_base[], as in
// pjd_k_idct_colour; staged as decoded (pjd_k_dense_stage_body.h with PJD_DENSE_RAW).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_std_dense(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base,
                                                                         uint8_t *__restrict__ planes)
{
    __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
    __shared__ __attribute__((aligned(16))) uint32_t ws[PJD_IDCT_MAX_DU][WS_STRIDE];
    __shared__ uint16_t qn[3][64];
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];

    const PjdDevIdctWg wg = wgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t tid = threadIdx.x;
    const uint32_t dus = im.dus_per_mcu;
    const uint32_t n_du = wg.n_mcu * dus;
    if (tid < 192) qn[tid >> 6][tid & 63] = B.qtab[(size_t)wg.image * 192 + tid];
    pjd_fill_mcu_xy(mcu_xy, wg, im, tid);
    const int16_t *cbase = B.coef + (dense_base[wg.pad_] + (uint64_t)(wg.first_mcu - im.first_mcu) * dus) * 64;
    const bool sentinel = !(im.flags & PJD_IF_PROGRESSIVE);
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) {
        const uint32_t du = i >> 3, r = i & 7;
        const int4 raw = *reinterpret_cast<const int4 *>(cbase + (size_t)du * 64 + r * 8);
#define PJD_DENSE_RAW
#include "pjd_k_dense_stage_body.h"
#undef PJD_DENSE_RAW
    }
    __syncthreads();
    pjd_std_idct_to_planes(tile, ws, qn, mcu_xy, im, n_du, planes, tid);
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
    const PjdStdPlanes P = pjd_std_planes(planes, im);
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
    uint32_t f[4], g[4], l[4];            // first / middle / last byte of a pixel: R, G, B -- B, G, R in the BMP image
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int r_, g_, b_;
        const int yy = (int)((yv >> (8 * k)) & 255);
        if (im.ncomp < 3) r_ = g_ = b_ = yy;
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

void pjd_launch_idct_std_lanes(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const uint32_t *order, uint32_t n_wg, uint8_t *planes)
{
    if (n_wg == 0) return;
    if (f.gray()) hipLaunchKernelGGL(pjd_gray_lanes_kernel(PJD_GRAY_LIBJPEG), dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, order);
    else hipLaunchKernelGGL(pjd_k_idct_std_lanes, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, order, planes);
}

void pjd_launch_idct_std_dense(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const PjdDevIdctWg *wgs, const uint64_t *dense_base, uint32_t n_wg, uint8_t *planes)
{
    if (n_wg == 0) return;
    if (f.gray()) hipLaunchKernelGGL(pjd_gray_dense_kernel(PJD_GRAY_LIBJPEG), dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, wgs, dense_base);
    else hipLaunchKernelGGL(pjd_k_idct_std_dense, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, wgs, dense_base, planes);
}

void pjd_launch_colour_std(hipStream_t s, const PjdDevBatch &b, const PjdDevIdctWg *cwgs, uint32_t n_wg, uint8_t *planes)
{
    if (n_wg) hipLaunchKernelGGL(pjd_k_colour_std, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, cwgs, planes);
}
