// pjd_k_backend_gray.hip -- the back end of a PJD_OUT_GRAY8 batch (include/pjd.h): one plane, uint8[H][W], the value R = G = B
// takes when every chroma sample is neutral.  Under the reference's arithmetic that is clamp255(Y + 128) of the luma sample after the
// reference's IDCT (src/decoder_dpu.c:376-382 with Cb = Cr = 0), under PJD_F_LIBJPEG libjpeg's own luma sample.
//
//   pjd_k_idct_gray_lanes<SCALED> / pjd_k_idct_gray<SCALED>
//                       the front ends of pjd_k_backend.hip -- the group parser of the lane streams (the same text, included, with
//                       PJD_LANES_LUMA_ONLY: chroma entries are walked, because the stream interleaves them, and dropped), the dense
//                       scratch of the exact kernel -- then DC prediction, row pass and column pass over the LUMA units alone, and the
//                       store: a lane takes the eight samples of one row of one unit and writes them as one 8-byte store (bytes at the
//                       ragged right edge).  SCALED: pictures with PJD_F_SCALE_* take the box filter of include/pjd.h on the one plane;
//                       a box of 2, 4 or 8 pixels a side lies inside one luma unit.
//   pjd_k_idct_gray_std_lanes[_red] / pjd_k_idct_gray_std_dense[_red]
//                       PJD_F_LIBJPEG pictures: jpeg_idct_islow of the luma units (pjd_libjpeg.h) -- _red: libjpeg's reduced IDCT, for the
//                       pictures with PJD_F_LIBJPEG_SCALE_* -- straight into the picture, clipped to its width and height.  No component
//                       planes, no chroma, no colour launch.  A kernel and its _red twin share their front end: pjd_gray_std_lanes<RED>,
//                       and pjd_k_libjpeg_dense_body.h with PJD_LJ_LUMA_ONLY (the text of pjd_k_backend_std.hip's dense kernels too).
// Kernels of their own, as the planar and the scaled back ends are.  Of their own are the stores and pjd_gray_dc; the walk over the luma
// units (PjdLumaUnits), the parser, the dense staging, the IDCT passes and the islow passes are the texts the other units use
// (pjd_k_backend_common.h, pjd_k_dense_stage_body.h, pjd_libjpeg_passes.h).  No launcher here: those of pjd_k_backend.hip and
// pjd_k_backend_std.hip take the kernels from the two accessors at the end.
#include "pjd_libjpeg_passes.h"

namespace {

struct __attribute__((packed)) PjdPx8 { uint32_t a, b; };

// eight int16 luma samples (four dwords) -> eight bytes clamp255(y + 128): the int16 sum saturates only outside [0, 255]
__device__ __forceinline__ uint2 pjd_gray_bytes(const uint4 w)
{
    uint2 r;
    r.x = pjd_sat_pk_u8_i16(pjd_pk_add_i16_sat(w.x, 0x00800080u));
    pjd_sat_pk_u8_i16_hi(r.x, pjd_pk_add_i16_sat(w.y, 0x00800080u));
    r.y = pjd_sat_pk_u8_i16(pjd_pk_add_i16_sat(w.z, 0x00800080u));
    pjd_sat_pk_u8_i16_hi(r.y, pjd_pk_add_i16_sat(w.w, 0x00800080u));
    return r;
}

// eight adjacent bytes of one picture row from column X on, cut at the right picture edge (X < width).  The wide stores go to ANY
// address: a picture starts at whatever byte the caller bound (pjd_batch_bind_output promises no alignment for uint8), rows are W bytes
// apart, and gfx950 global stores need no alignment -- the packed structs say so to the compiler, as PjdPx4 / PjdPx12 do for the planar
// and interleaved stores.  So an unaligned destination takes the same 8-byte store and NOT a run of byte stores; byte stores are used
// only for the one to three pixels in front of the right edge.  tests/test_gpu_gray.py binds at an odd address between canary bytes.
__device__ __forceinline__ void pjd_gray_store8(uint8_t *o, const uint2 px, uint32_t X, uint32_t width)
{
    if (X + 8 <= width) {
        PjdPx8 v; v.a = px.x; v.b = px.y;
        *reinterpret_cast<PjdPx8 *>(o) = v;
        return;
    }
    const uint32_t n = width - X;                              // 1..7
    uint32_t lo = px.x;
    if (n >= 4) { reinterpret_cast<PjdPx4 *>(o)->a = lo; o += 4; lo = px.y; }
    for (uint32_t k = 0; k < (n & 3u); k++) o[k] = (uint8_t)(lo >> (8 * k));
}

// Full-size store of the luma units in `tile` (both passes done).  A wave sweeps picture rows of the range's MCUs: consecutive lanes
// take consecutive units of one row, so that a store instruction covers runs of it; where the range has few units per row a wave takes
// several rows at once.  No division: everything is a shift of a power of two.
__device__ __forceinline__ void pjd_gray_store(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, uint8_t *out, const PjdDevImage &im,
                                               uint32_t n_mcu, uint32_t tid)
{
    const uint32_t width = im.width, height = im.height, stride = im.out_stride, hs = im.hs, vs = im.vs, dus = im.dus_per_mcu;
    const uint32_t hs_log = hs - 1u, mh = 8u * vs;
    const uint32_t per_row = n_mcu << hs_log;                  // units side by side in the range (1..96)
    uint32_t lp = 32u - (uint32_t)__builtin_clz(per_row | 1u); // lanes of a wave that share one row: the next power of two, at most 64
    if ((1u << (lp - 1u)) >= per_row) lp--;
    if (lp > 6u) lp = 6u;
    const uint32_t lane = tid & 63u, wv = tid >> 6, rows = 64u >> lp;
    for (uint32_t py = wv * rows + (lane >> lp); py < mh; py += (PJD_IDCT_THREADS / 64) * rows) {
        for (uint32_t idx = lane & ((1u << lp) - 1u); idx < per_row; idx += 1u << lp) {
            const uint32_t ml = idx >> hs_log, cg = idx & (hs - 1u);
            const uint32_t xy = mcu_xy[ml];
            const uint32_t X = (__umul24(xy & 0xffffu, hs) + cg) * 8u, Y = __umul24(xy >> 16, mh) + py;
            if (X >= width || Y >= height) continue;
            const uint32_t u = __umul24(ml, dus) + (py >> 3) * hs + cg;
            const uint4 w = *reinterpret_cast<const uint4 *>(&tile[u][(py & 7u) * 8u]);
            pjd_gray_store8(out + (size_t)Y * stride + X, pjd_gray_bytes(w), X, width);
        }
    }
}

// Reduced-size store (PJD_F_SCALE_*): output pixel (i, j) is the rounded mean of the bytes clamp255(y + 128) of the source box
// [S*i, S*i + S) x [S*j, S*j + S), cut at the right and bottom picture edge -- the box filter of include/pjd.h on the one plane.  S divides
// 8, so a box lies inside one luma unit: a thread takes one box row of one unit, 8 / S output pixels.
template <int S>
__device__ __forceinline__ void pjd_gray_store_scaled(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, uint8_t *out, const PjdDevImage &im,
                                                      uint32_t n_mcu, uint32_t tid)
{
    constexpr uint32_t S_LOG = S == 2 ? 1 : (S == 4 ? 2 : 3), BR_LOG = 3 - S_LOG;
    constexpr int NO = 8 / S;
    const uint32_t width = im.width, height = im.height, stride = im.out_stride, hs = im.hs, vs = im.vs;
    const PjdLumaUnits L = pjd_luma_units(im);
    const uint32_t tasks = (n_mcu * L.nl) << BR_LOG;
    for (uint32_t t = tid; t < tasks; t += PJD_IDCT_THREADS) {
        const uint32_t j = t >> BR_LOG, br = t & ((1u << BR_LOG) - 1u);
        const uint2 at = pjd_luma_unit_xy(j, L, hs, vs, mcu_xy, 8u);
        const uint32_t X = at.x, Yb = at.y + br * S;
        if (X >= width || Yb >= height) continue;
        const uint32_t u = pjd_luma_unit(j, L);
        const uint32_t bh = height - Yb < S ? height - Yb : S;
        uint32_t sum[NO];
#pragma unroll
        for (int q = 0; q < NO; q++) sum[q] = 0;
#pragma unroll
        for (uint32_t v = 0; v < S; v++) {
            if (v >= bh) break;
            const uint2 b = pjd_gray_bytes(*reinterpret_cast<const uint4 *>(&tile[u][(br * S + v) * 8u]));
#pragma unroll
            for (int p = 0; p < 8; p++) {
                const uint32_t s = ((p < 4 ? b.x : b.y) >> (8 * (p & 3))) & 255u;
                sum[p / S] += (p == 0 || X + p < width) ? s : 0u;          // pixels past the right edge do not count
            }
        }
        uint8_t *o = out + (size_t)(Yb >> S_LOG) * stride + (X >> S_LOG);
        uint32_t px = 0;
        int n_out = 0;
#pragma unroll
        for (int q = 0; q < NO; q++) {
            const uint32_t bx = X + q * S;                      // first column of the box
            if (q > 0 && bx >= width) break;
            const uint32_t n = (width - bx < S ? width - bx : S) * bh;
            const uint32_t a = n == S * S ? (sum[q] + S * S / 2) >> (2 * S_LOG) : (sum[q] + (n >> 1)) / n;
            px |= a << (8 * q);
            n_out = q + 1;
        }
        if (NO == 4 && n_out == 4) reinterpret_cast<PjdPx4 *>(o)->a = px;
        else for (int q = 0; q < n_out; q++) o[q] = (uint8_t)(px >> (8 * q));
    }
}

template <bool SCALED>
__device__ __forceinline__ void pjd_gray_dispatch(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, const PjdDevBatch &B, const PjdDevImage &im,
                                                  uint32_t n_mcu, uint32_t tid)
{
    uint8_t *out = B.out + im.out_off;
    if (SCALED) {
        switch ((im.flags & PJD_IF_SCALE_MASK) >> PJD_IF_SCALE_SHIFT) {
            case 1: pjd_gray_store_scaled<2>(tile, mcu_xy, out, im, n_mcu, tid); return;
            case 2: pjd_gray_store_scaled<4>(tile, mcu_xy, out, im, n_mcu, tid); return;
            case 3: pjd_gray_store_scaled<8>(tile, mcu_xy, out, im, n_mcu, tid); return;
            default: break;
        }
    }
    pjd_gray_store(tile, mcu_xy, out, im, n_mcu, tid);
}

// DC prediction of the LUMA units of a range by wave 0: the differences the parser left in tile[u][0] become absolute values, scaled
// by the quantiser in qz (all modulo 2^16).  A restart head is the first unit of an MCU, which is a luma unit.  This is
// pjd_k_lanes_dc_body.h with the chroma sums taken out, kept as a copy: that body with a luma-only switch did not compile to this
// text in the three lane kernels below (profiles/backend_shared_stages.md).
__device__ __forceinline__ void pjd_gray_dc(int16_t (*tile)[TILE_STRIDE], const uint32_t (*qz)[64], const uint8_t *comp_of, const uint8_t *du_head,
                                            uint32_t pred0y, uint32_t n_du, uint32_t n_valid, uint32_t lane)
{
    uint32_t cy = (pred0y * (qz[0][0] & 0xffffu)) & 0xffffu;   // the predictor entering the next group of 64 units
    for (uint32_t base = 0; base < n_du; base += 64) {
        const uint32_t u = base + lane;
        const bool on = u < n_valid;                            // an undecoded unit keeps DC 0: it is never predicted
        const uint32_t us = on ? u : 0u;
        const bool luma = on && comp_of[us] == 0;
        const uint32_t dv = luma ? (uint32_t)(uint16_t)tile[us][0] : 0u;
        const bool head = on && du_head[us] != 0;
        uint32_t vy = dv;
        PJD_WAVE_SCAN(pjd_op_add, vy);
        uint32_t hpos = head ? lane + 1 : 0u;                   // 1 + lane of the last head at or before this unit
        PJD_WAVE_SCAN(pjd_op_max, hpos);
        const uint32_t hl = hpos ? hpos - 1 : 0u;
        const uint32_t by = __shfl(vy, (int)hl) - __shfl(dv, (int)hl);     // a head resets the predictor BEFORE its own difference is added
        const uint32_t ty = hpos ? vy - by : vy + cy;
        if (luma) tile[u][0] = (int16_t)ty;
        cy = __shfl(ty, 63);
    }
}

// One back-end range of the lane streams by the whole workgroup; the LDS arrays are the kernel's.
template <bool SCALED>
__device__ __forceinline__ void pjd_gray_range(const PjdDevBatch &B, uint32_t iwg, int16_t (*tile)[TILE_STRIDE], uint32_t (*qz)[64], uint32_t *mcu_xy,
                                               uint8_t *comp_of, uint8_t *du_head, uint32_t *wagg, uint32_t *ltab)
{
#define PJD_LANES_LUMA_ONLY
#include "pjd_k_lanes_parse_body.h"
#undef PJD_LANES_LUMA_ONLY
    const PjdLumaUnits L = pjd_luma_units(dus, nl);
    const uint32_t n_lu = wg.n_mcu * nl;
    // DC prediction by wave 0, while the other waves do the row pass of rows 1..7 (only row 0 holds the DC coefficient) and the slot-52
    // rule (natural 38 lies in row 4) -- of the luma units alone
    if (wv != 0) {
        for (uint32_t i = tid - 64; i < n_lu * 7; i += PJD_IDCT_THREADS - 64) {
            const uint32_t j = pjd_div_small(i, c_recip16[7]), r = 1 + (i - __umul24(j, 7u));   // i < 7 * PJD_IDCT_MAX_DU: exact
            const uint32_t u = pjd_luma_unit(j, L);
            if (r == 4 && tile[u][64] != (int16_t)PJD_COEF_SENTINEL) tile[u][38] = (int16_t)pjd_dequant((int)tile[u][64], qz[0][48] & 0xffffu);
            pjd_tile_row(tile, u, r);
        }
    } else {
        pjd_gray_dc(tile, qz, comp_of, du_head, pred0[0], n_du, n_valid, lane);
    }
    __syncthreads();
    for (uint32_t j = tid; j < n_lu; j += PJD_IDCT_THREADS) pjd_tile_row(tile, pjd_luma_unit(j, L), 0);
    __syncthreads();
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) pjd_tile_col(tile, pjd_luma_unit(i >> 3, L), i & 7);
    __syncthreads();
    pjd_gray_dispatch<SCALED>(tile, mcu_xy, B, im, wg.n_mcu, tid);
}

// jpeg_idct_islow of the luma units staged in `tile` (natural order, as decoded) and the store of their samples into the picture,
// clipped to its width and height: the two passes of pjd_k_backend_std.hip, whose component planes a grey picture does not need.
__device__ __forceinline__ void pjd_gray_std_idct(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t *q, const uint32_t *mcu_xy,
                                                  const PjdDevBatch &B, const PjdDevImage &im, uint32_t n_mcu, uint32_t tid)
{
    const PjdLumaUnits L = pjd_luma_units(im);
    const uint32_t hs = im.hs, vs = im.vs, n_lu = n_mcu * L.nl;
    // pass 1: a thread takes one column of one unit
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) {
        const uint32_t u = pjd_luma_unit(i >> 3, L), c = i & 7;
        PJD_LJ_PASS1_COL(tile, ws, u, q, c);
    }
    __syncthreads();
    // pass 2: a thread takes one row of one unit and stores its 8 samples
    const uint32_t width = im.width, height = im.height, stride = im.out_stride;
    uint8_t *out = B.out + im.out_off;
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) {
        const uint32_t j = i >> 3, r = i & 7, u = pjd_luma_unit(j, L);
        const uint2 at = pjd_luma_unit_xy(j, L, hs, vs, mcu_xy, 8u);
        const uint32_t X = at.x, Y = at.y + r;
        if (X >= width || Y >= height) continue;
        const uint2 px = pjd_lj_pass2_row(ws, u, r);
        pjd_gray_store8(out + (size_t)Y * stride + X, px, X, width);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Lane-stream front end: one workgroup = one back-end range, as in pjd_k_idct_colour_lanes.
// order: the launch's workgroup -> index into PjdDevBatch::iwgs / marks (null: the identity, one launch for the whole batch)
// ---------------------------------------------------------------------------------------------
template <bool SCALED>
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray_lanes(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    PJD_LANES_LDS

#if PJD_IDCT_PRIO
    __builtin_amdgcn_s_setprio(PJD_IDCT_PRIO);
#endif
    pjd_gray_range<SCALED>(B, order ? order[blockIdx.x] : blockIdx.x, tile, qz, mcu_xy, comp_of, du_head, wagg, ltab);
}

// ---------------------------------------------------------------------------------------------
// Dense front end (pictures of the exact kernel and progressive frames): wgs[k].pad_ = index into dense_base[], as in
// pjd_k_idct_colour; the scratch is read the same way (pjd_k_idct_dense_body.h), the luma units alone.
// ---------------------------------------------------------------------------------------------
template <bool SCALED>
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base)
{
    __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
    __shared__ uint16_t qs[64];
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];

    const PjdDevIdctWg wg = wgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t tid = threadIdx.x;
    const PjdLumaUnits L = pjd_luma_units(im);
    const uint32_t dus = L.dus, n_lu = wg.n_mcu * L.nl;

    if (tid < 64) qs[tid] = B.qtab[(size_t)wg.image * 192 + tid];
    pjd_fill_mcu_xy(mcu_xy, wg, im, tid);
    __syncthreads();

    // load (16 B per lane), de-zigzag, dequantise: lane (unit, r) owns zigzag slots 8r..8r+7
    const int16_t *cbase = B.coef + (dense_base[wg.pad_] + (uint64_t)(wg.first_mcu - im.first_mcu) * dus) * 64;
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) {
        const uint32_t du = pjd_luma_unit(i >> 3, L), r = i & 7;
        const int4 raw = *reinterpret_cast<const int4 *>(cbase + (size_t)du * 64 + r * 8);
#define PJD_DENSE_Q qs
#include "pjd_k_dense_stage_body.h"
#undef PJD_DENSE_Q
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) pjd_tile_row(tile, pjd_luma_unit(i >> 3, L), i & 7);
    __syncthreads();
    for (uint32_t i = tid; i < n_lu * 8; i += PJD_IDCT_THREADS) pjd_tile_col(tile, pjd_luma_unit(i >> 3, L), i & 7);
    __syncthreads();
    pjd_gray_dispatch<SCALED>(tile, mcu_xy, B, im, wg.n_mcu, tid);
}

// ---------------------------------------------------------------------------------------------
// PJD_F_LIBJPEG pictures of a grey batch, from the lane streams and from the dense scratch.  RED: the pictures with PJD_F_LIBJPEG_SCALE_*,
// whose luma units go through libjpeg's reduced IDCT of M = 4, 2 or 1 samples a side (PjdLjRed<M>, pjd_libjpeg.h), straight into the
// picture, clipped at its reduced width and height; M is the picture's, uniform over the workgroup.  Each front end is one text, the
// body of its two kernels, which differ in the passes behind it.
// ---------------------------------------------------------------------------------------------
namespace {

struct __attribute__((packed)) PjdPx2 { uint16_t a; };

template <int M>
__device__ __forceinline__ void pjd_gray_red_idct(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t *q, const uint32_t *mcu_xy,
                                                  const PjdDevBatch &B, const PjdDevImage &im, uint32_t n_mcu, uint32_t tid)
{
    constexpr uint32_t M_LOG = M == 4 ? 2 : (M == 2 ? 1 : 0), COLS = M == 4 ? 7 : 5;
    const PjdLumaUnits L = pjd_luma_units(im);
    const uint32_t hs = im.hs, vs = im.vs, n_lu = n_mcu * L.nl;
    if (M > 1) {
        // pass 1: a thread takes one of the columns the transform reads of one unit
        for (uint32_t i = tid; i < n_lu * COLS; i += PJD_IDCT_THREADS) {
            const uint32_t j = pjd_div_small(i, c_recip16[COLS]), k = i - j * COLS;     // i < 7 * PJD_IDCT_MAX_DU: exact
            pjd_lj_red_pass1_col<(M == 2 ? 2 : 4)>(tile, ws, pjd_luma_unit(j, L), q, k);
        }
        __syncthreads();
    }
    // pass 2: a thread takes one row of one unit and stores its M samples
    const uint32_t width = (im.width + 8u / M - 1u) >> (3u - M_LOG), height = (im.height + 8u / M - 1u) >> (3u - M_LOG), stride = im.out_stride;
    uint8_t *out = B.out + im.out_off;
    for (uint32_t i = tid; i < (n_lu << M_LOG); i += PJD_IDCT_THREADS) {
        const uint32_t j = i >> M_LOG, r = i & (M - 1u), u = pjd_luma_unit(j, L);
        const uint2 at = pjd_luma_unit_xy(j, L, hs, vs, mcu_xy, M);
        const uint32_t X = at.x, Y = at.y + r;
        if (X >= width || Y >= height) continue;
        uint8_t *o = out + (size_t)Y * stride + X;
        if (M == 1) { *o = (uint8_t)pjd_lj_sample_1x1(pjd_lj_dequant((int)tile[u][0], q[0])); continue; }
        const uint32_t px = pjd_lj_red_pass2_row<(M == 2 ? 2 : 4)>(ws, u, r);
        // one store of the row's samples to ANY address (pjd_gray_store8); bytes in front of the right edge
        if (X + M <= width) {
            if (M == 4) reinterpret_cast<PjdPx4 *>(o)->a = px;
            else reinterpret_cast<PjdPx2 *>(o)->a = (uint16_t)px;
        } else {
            for (uint32_t p = 0; p < width - X; p++) o[p] = (uint8_t)(px >> (8 * p));
        }
    }
}

__device__ __forceinline__ void pjd_gray_red_dispatch(const int16_t (*tile)[TILE_STRIDE], uint32_t (*ws)[WS_STRIDE], const uint16_t *q, const uint32_t *mcu_xy,
                                                      const PjdDevBatch &B, const PjdDevImage &im, uint32_t n_mcu, uint32_t tid)
{
    switch ((im.flags & PJD_IF_LJSCALE_MASK) >> PJD_IF_LJSCALE_SHIFT) {
        case 1: pjd_gray_red_idct<4>(tile, ws, q, mcu_xy, B, im, n_mcu, tid); break;
        case 2: pjd_gray_red_idct<2>(tile, ws, q, mcu_xy, B, im, n_mcu, tid); break;
        case 3: pjd_gray_red_idct<1>(tile, ws, q, mcu_xy, B, im, n_mcu, tid); break;
        default: break;                                         // never: the planner sends full-size pictures to the kernels above
    }
}

template <bool RED>
__device__ __forceinline__ void pjd_gray_std_lanes(const PjdDevBatch &B, const uint32_t *order)
{
    PJD_LANES_LDS_TILE
    __shared__ __attribute__((aligned(16))) uint32_t ws[PJD_IDCT_MAX_DU][WS_STRIDE];
    __shared__ uint16_t qn[64];               // the luma quantiser by natural position
    PJD_LANES_LDS_TABLES                      // qz here: 1 | natural position << 16 (the parser stores what was decoded)

    const uint32_t iwg = order[blockIdx.x];
    if (threadIdx.x < 64) qn[threadIdx.x] = B.qtab[(size_t)B.iwgs[iwg].image * 192 + threadIdx.x];
#define PJD_LANES_RAW
#define PJD_LANES_LUMA_ONLY
#include "pjd_k_lanes_parse_body.h"
#undef PJD_LANES_LUMA_ONLY
#undef PJD_LANES_RAW
    if (wv == 0) pjd_gray_dc(tile, qz, comp_of, du_head, pred0[0], n_du, n_valid, lane);
    __syncthreads();
    if (RED) pjd_gray_red_dispatch(tile, ws, qn, mcu_xy, B, im, wg.n_mcu, tid);
    else pjd_gray_std_idct(tile, ws, qn, mcu_xy, B, im, wg.n_mcu, tid);
}

}  // namespace

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray_std_lanes(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    pjd_gray_std_lanes<false>(B, order);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray_std_lanes_red(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    pjd_gray_std_lanes<true>(B, order);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray_std_dense(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base)
{
#define PJD_LJ_LUMA_ONLY
#include "pjd_k_libjpeg_dense_body.h"
#undef PJD_LJ_LUMA_ONLY
    pjd_gray_std_idct(tile, ws, qn, mcu_xy, B, im, wg.n_mcu, tid);
}

__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_gray_std_dense_red(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base)
{
#define PJD_LJ_LUMA_ONLY
#include "pjd_k_libjpeg_dense_body.h"
#undef PJD_LJ_LUMA_ONLY
    pjd_gray_red_dispatch(tile, ws, qn, mcu_xy, B, im, wg.n_mcu, tid);
}

// the grey kernels, scaled / full size / PJD_F_LIBJPEG / PJD_F_LIBJPEG_SCALE_*: the launchers of the forms stand in pjd_k_backend.hip and
// pjd_k_backend_std.hip
PjdLanesKernel pjd_gray_lanes_kernel(PjdGrayKernel which)
{
    static const PjdLanesKernel k[4] = {pjd_k_idct_gray_lanes<true>, pjd_k_idct_gray_lanes<false>, pjd_k_idct_gray_std_lanes, pjd_k_idct_gray_std_lanes_red};
    return k[which];
}

PjdDenseKernel pjd_gray_dense_kernel(PjdGrayKernel which)
{
    static const PjdDenseKernel k[4] = {pjd_k_idct_gray<true>, pjd_k_idct_gray<false>, pjd_k_idct_gray_std_dense, pjd_k_idct_gray_std_dense_red};
    return k[which];
}
