// pjd_k_backend.hip -- gfx950 kernels behind the entropy decoder:
//
//   pjd_k_dpu_payload   the reference's per-DPU contract, one workgroup per 16x16 "block"
//                       (reference src/decoder_dpu.c:82-390)
//   pjd_k_reset / _zero per-decode state reset (kernels of ours, not runtime memset nodes)
//   pjd_k_lane_dc_local /  DC prediction: the entropy decoder leaves DC DIFFERENCES and per-lane sums; the predictors at every
//   pjd_k_lane_dc_carry    lane start are a two-level segmented scan over lanes (reference src/jpeg_scanner.cpp:485-486,723-727)
//   pjd_k_idct_colour_lanes / pjd_k_idct_colour
//                       fused de-zigzag + dequantise + 8x8 IDCT + chroma upsample + YCbCr->RGB + raster / BMP store
//                       (reference src/decoder_dpu.c:158-390 and src/bmp_writer.cpp:43-65 for the BMP row order).
//                       _lanes parses the parallel decoder's lane streams (one 16-bit entry per symbol, one or two per
//                       step word); the other reads the dense int16 scratch the exact kernel fills.
//   pjd_k_idct_colour_lanes_planar / pjd_k_idct_colour_planar
//                       the same two for a PJD_OUT_RGB8_PLANAR batch: R, G and B go to three planes (uint8[3][H][W]); kernels of
//                       their own, so that the interleaved ones keep their code
// What these kernels share with the other two back-end units stands once, in pjd_k_backend_common.h (LDS block, MCU positions, the two
// IDCT passes) and in the bodies they include (pjd_k_lanes_parse_body.h, pjd_k_lanes_dc_body.h, pjd_k_idct_dense_body.h with
// pjd_k_dense_stage_body.h).  pjd_launch_idct_lanes and pjd_launch_idct_dense pick the kernel of a batch's form (PjdBackForm), the grey
// unit's included.
//
// Integer work bound by VALU instruction issue (profiles/r03_cfg3.md: valu_issue_frac 1.0 -- the entry parser is its largest
// phase), not by HBM: coefficients are read once with 16-byte loads, tiles live in LDS (row stride 144 B so that the column
// pass is bank-conflict free), pictures are written once.
#include "pjd_k_backend_common.h"


// ---------------------------------------------------------------------------------------------
// Literal DPU payload: metadata u32[276] + mcus i16[19200] per DPU.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void pjd_k_dpu_payload(const uint32_t *__restrict__ meta_all, int16_t *__restrict__ mcus_all)
{
    __shared__ __attribute__((aligned(16))) int16_t tile[12][TILE_STRIDE];   // [comp*4 + pos][64]
    const int dpu = blockIdx.x / 25, blk = blockIdx.x % 25;
    const uint32_t *m = meta_all + (size_t)dpu * 276;
    int16_t *base = mcus_all + (size_t)dpu * 19200 + blk * 768;
    const int tid = threadIdx.x;
    const int ncomp = (int)m[4];
    const int V = (int)(m[5] & 255), H = (int)(m[6] & 255);

    // dequantise (decoder_dpu.c:158-177) and row pass (:218-268): lane owns one row
    if (tid < 96) {
        const int du = tid >> 3, r = tid & 7, comp = du >> 2;
        const int4 raw = *reinterpret_cast<const int4 *>(base + du * 64 + r * 8);
        const int16_t *rv = reinterpret_cast<const int16_t *>(&raw);
        int x[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = rv[j];
        if (comp < ncomp) {
            const uint32_t *q = m + 20 + (m[7 + comp] & 255) * 64 + r * 8;
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = pjd_dequant(x[j], q[j]);
        }
        pjd_idct8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], o);
#pragma unroll
        for (int j = 0; j < 8; j++) tile[du][r * 8 + j] = (int16_t)o[j];
    }
    __syncthreads();
    // column pass (decoder_dpu.c:270-320)
    if (tid < 96) {
        const int du = tid >> 3, c = tid & 7;
        int x[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = tile[du][j * 8 + c];
        pjd_idct8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], o);
#pragma unroll
        for (int j = 0; j < 8; j++) tile[du][j * 8 + c] = (int16_t)o[j];
    }
    __syncthreads();
    // colour (decoder_dpu.c:323-390).  (cbcr_index, v, h) per position follow the four tuples
    // of each sampling mode; all reads come from LDS, all writes go to HBM, so the
    // reference's in-place ordering constraints disappear.
    for (int i = tid; i < 256; i += 128) {
        const int pos = i >> 6, p = i & 63, y = p >> 3, x = p & 7;
        int cidx, v, h;
        if (V == 1 && H == 1)      { cidx = pos;     v = 0;        h = 0; }
        else if (V == 2 && H == 1) { cidx = pos & 1; v = pos >> 1; h = 0; }
        else if (V == 1 && H == 2) { cidx = pos & 2; v = 0;        h = pos & 1; }
        else                       { cidx = 0;       v = pos >> 1; h = pos & 1; }
        const int q = ((y / V) + 4 * v) * 8 + (x / H) + 4 * h;
        int r, g, b;
        pjd_ycc_to_rgb(tile[pos][p], tile[4 + cidx][q], tile[8 + cidx][q], r, g, b);
        base[pos * 64 + p] = (int16_t)r;
        base[256 + pos * 64 + p] = (int16_t)g;
        base[512 + pos * 64 + p] = (int16_t)b;
    }
}

// ---------------------------------------------------------------------------------------------
// Per-decode reset: status words from their initial values (images routed to the exact kernel start flagged), the
// statistics, the words the Huffman waves publish to each other, the debug timeline.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pjd_k_reset(PjdDevBatch B, const int32_t *__restrict__ status_init, uint64_t *__restrict__ opstate,
                                                   uint32_t opstate_words, uint32_t dbg_words)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < B.n_images) {
        B.status[i] = status_init[i];
        PjdDevImState st; st.err_key = ~0ull; st.flag_pos = 0xffffffffu; st.end_pos = 0xffffffffu;
        B.imstate[i] = st;
    }
    if (i < 16) B.stats[i] = 0;
    if (i < opstate_words) opstate[i] = 0;
    for (uint32_t k = i; k < dbg_words; k += gridDim.x * 256) B.dbg[k] = 0;
}

__global__ __launch_bounds__(256) void pjd_k_zero(uint4 *__restrict__ p, uint64_t n16)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

void pjd_launch_zero(hipStream_t s, void *p, size_t bytes)
{
    const uint64_t n16 = bytes / 16;
    if (!n16) return;
    const uint64_t blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(pjd_k_zero, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, (uint4 *)p, n16);
}

void pjd_launch_reset(hipStream_t s, const PjdDevBatch &b, const int32_t *status_init, uint64_t *opstate, size_t opstate_words, uint32_t dbg_words)
{
    size_t n = b.n_images > 16 ? b.n_images : 16;
    if (opstate_words > n) n = opstate_words;
    hipLaunchKernelGGL(pjd_k_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b, status_init, opstate, (uint32_t)opstate_words, dbg_words);
}

void pjd_launch_dpu_payload(hipStream_t s, const uint32_t *metadata, int16_t *mcus, int n_dpus)
{
    hipLaunchKernelGGL(pjd_k_dpu_payload, dim3(n_dpus * 25), dim3(128), 0, s, metadata, mcus);
}

// ---------------------------------------------------------------------------------------------
// DC prediction.  The entropy decoder emits DC DIFFERENCES and, per lane, their sum per component.
// The predictors at the start of every lane are a segmented scan over lanes (a lane that starts a
// restart segment resets them, reference src/jpeg_scanner.cpp:485-486,723-727), done in two levels:
// blocks of PJD_DC_BLOCK lanes, then one workgroup over the block aggregates.  The back end adds
// the block's carry-in itself.  All sums are modulo 2^16 like the reference's `short` stores.
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Per-picture verdict of the parallel entropy decode (after pjd_k_huff_lanes, before the back end): the first entropy-coding
// error of the true decode gives the status word -- the reference's error class; its picture keeps what was decoded before the
// error (reference src/decoder_host.cpp:181 ignores the failure and writes the picture) -- unless something the decoder could
// not resolve lies at or before it: then, and for any unresolved thing in a picture without an error, the exact kernel decodes it.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pjd_k_image_verdict(PjdDevBatch B)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B.n_images) return;
    const int32_t st = B.status[i];
    if (st & PJD_STW_NEEDS_EXACT) return;                       // routed to the exact kernel up front
    const PjdDevImState s = B.imstate[i];
    const bool has_err = s.err_key != ~0ull;
    const uint32_t err_pos = (uint32_t)(s.err_key >> 32);
    const bool flagged = s.flag_pos != 0xffffffffu && s.flag_pos <= s.end_pos;      // not behind the picture's last unit (pjd_internal.h)
    if (flagged && (!has_err || s.flag_pos <= err_pos)) B.status[i] = st | PJD_STW_NEEDS_EXACT;
    else if (has_err) B.status[i] = (int32_t)((s.err_key >> 1) & 7u);
}


__global__ __launch_bounds__(PJD_DC_BLOCK) void pjd_k_lane_dc_local(PjdDevBatch B)
{
    __shared__ uint32_t sy[PJD_DC_BLOCK], scb[PJD_DC_BLOCK], scr[PJD_DC_BLOCK], sf[PJD_DC_BLOCK];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t q = b * PJD_DC_BLOCK + tid;
    uint32_t vy = 0, vcb = 0, vcr = 0, head = 0;
    if (q < B.n_lanes) {
        const PjdDevLaneInfo li = B.lane_info[q];
        vy = li.dc_sum[0]; vcb = li.dc_sum[1]; vcr = li.dc_sum[2]; head = li.first_du >> 31;
    }
    sy[tid] = vy; scb[tid] = vcb; scr[tid] = vcr; sf[tid] = head;
    __syncthreads();
    // Hillis-Steele inclusive segmented scan
    for (uint32_t off = 1; off < PJD_DC_BLOCK; off <<= 1) {
        uint32_t ay = 0, acb = 0, acr = 0, af = 0;
        const bool take = tid >= off;
        if (take) { ay = sy[tid - off]; acb = scb[tid - off]; acr = scr[tid - off]; af = sf[tid - off]; }
        const uint32_t myf = sf[tid];
        __syncthreads();
        if (take) {
            if (!myf) { sy[tid] += ay; scb[tid] += acb; scr[tid] += acr; }
            sf[tid] = myf | af;
        }
        __syncthreads();
    }
    if (q < B.n_lanes) {
        // predictors entering this lane: the inclusive result of the lane before it, zero at a segment head
        PjdDevLaneDc d;
        d.dc_in[0] = d.dc_in[1] = d.dc_in[2] = 0;
        d.abs = (uint16_t)(head | (tid > 0 ? sf[tid - 1] : 0u));
        if (!head && tid > 0) { d.dc_in[0] = (uint16_t)sy[tid - 1]; d.dc_in[1] = (uint16_t)scb[tid - 1]; d.dc_in[2] = (uint16_t)scr[tid - 1]; }
        B.lane_dc[q] = d;
    }
    if (tid == PJD_DC_BLOCK - 1) {
        uint16_t *agg = B.dc_blk + (size_t)b * 8;
        agg[0] = (uint16_t)sy[tid]; agg[1] = (uint16_t)scb[tid]; agg[2] = (uint16_t)scr[tid]; agg[3] = (uint16_t)sf[tid];
    }
}

// One workgroup: carry-in of every block = exclusive segmented scan of the block aggregates.
__global__ __launch_bounds__(256) void pjd_k_lane_dc_carry(PjdDevBatch B)
{
    __shared__ uint32_t sy[256], scb[256], scr[256], sf[256];
    const uint32_t tid = threadIdx.x, n = B.n_dcblk;
    uint32_t cy = 0, ccb = 0, ccr = 0;                       // predictors entering the current chunk of blocks
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t j = base + tid;
        uint32_t vy = 0, vcb = 0, vcr = 0, vf = 0;
        if (j < n) { const uint16_t *a = B.dc_blk + (size_t)j * 8; vy = a[0]; vcb = a[1]; vcr = a[2]; vf = a[3]; }
        sy[tid] = vy; scb[tid] = vcb; scr[tid] = vcr; sf[tid] = vf;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            uint32_t ay = 0, acb = 0, acr = 0, af = 0;
            const bool take = tid >= off;
            if (take) { ay = sy[tid - off]; acb = scb[tid - off]; acr = scr[tid - off]; af = sf[tid - off]; }
            const uint32_t myf = sf[tid];
            __syncthreads();
            if (take) {
                if (!myf) { sy[tid] += ay; scb[tid] += acb; scr[tid] += acr; }
                sf[tid] = myf | af;
            }
            __syncthreads();
        }
        if (j < n) {
            // exclusive: what the blocks before j leave behind
            uint32_t iy = cy, icb = ccb, icr = ccr;
            if (tid > 0) {
                const bool h = sf[tid - 1] != 0;
                iy = (h ? 0u : cy) + sy[tid - 1]; icb = (h ? 0u : ccb) + scb[tid - 1]; icr = (h ? 0u : ccr) + scr[tid - 1];
            }
            uint16_t *c = B.dc_blk + (size_t)j * 8 + 4;
            c[0] = (uint16_t)iy; c[1] = (uint16_t)icb; c[2] = (uint16_t)icr; c[3] = 0;
        }
        const bool h = sf[255] != 0;
        const uint32_t ny = (h ? 0u : cy) + sy[255], ncb = (h ? 0u : ccb) + scb[255], ncr = (h ? 0u : ccr) + scr[255];
        __syncthreads();
        cy = ny; ccb = ncb; ccr = ncr;
    }
}

// Row pass, column pass, chroma upsample + colour + raster store for the data units staged in `tile`
// (natural order, dequantised).  Shared by the sparse and the dense front ends.
// DO_IDCT = false: the caller has already run both passes on every unit (and this function's first barrier is
// the one that separates them from the colour stage).  SCALED: pictures with an output scale take the scaled store (below).
// PLANAR: the batch's output format is PJD_OUT_RGB8_PLANAR (never BMP): the three channels of a pixel go to three planes.
template <bool PLANAR = false>
__device__ __forceinline__ void pjd_colour_dispatch_scaled(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, const PjdDevBatch &B,
                                                           const PjdDevImage &im, const PjdDevIdctWg &wg, uint32_t tid);
template <bool DO_IDCT, bool SCALED, bool PLANAR = false>
__device__ __forceinline__ void pjd_tile_to_pixels(int16_t (*tile)[TILE_STRIDE], uint32_t *mcu_xy, const PjdDevBatch &B,
                                                   const PjdDevImage &im, const PjdDevIdctWg &wg, uint32_t tid)
{
    pjd_fill_mcu_xy(mcu_xy, wg, im, tid);
    const uint32_t dus = im.dus_per_mcu, nl = im.n_luma, nc = im.ncomp, hs = im.hs, vs = im.vs;
    const uint32_t n_du = wg.n_mcu * dus;
    __syncthreads();
    if (DO_IDCT) {
        for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) pjd_tile_row(tile, i >> 3, i & 7);
        __syncthreads();
        for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) pjd_tile_col(tile, i >> 3, i & 7);
        __syncthreads();
    }
    if (SCALED && (im.flags & PJD_IF_SCALE_MASK)) { pjd_colour_dispatch_scaled<PLANAR>(tile, mcu_xy, B, im, wg, tid); return; }

    // ---- chroma upsample (nearest neighbour, decoder_dpu.c:370), colour, raster store --------
    const uint32_t mw = 8 * hs, mh = 8 * vs;
    const bool bmp = !PLANAR && (im.flags & PJD_IF_BMP) != 0;
    uint8_t *out = B.out + im.out_off;
    // image constants in registers: read through `im` they are re-fetched from HBM after every store
    const uint32_t width = im.width, height = im.height, stride = im.out_stride;
    if (bmp && wg.first_mcu == 0 && tid < 26) {
        // file header exactly as reference src/bmp_writer.cpp:32-41
        const uint32_t size = 26 + im.height * im.out_stride;
        uint8_t hb = 0;
        switch (tid) {
            case 0: hb = 'B'; break;  case 1: hb = 'M'; break;
            case 2: hb = size & 255; break; case 3: hb = (size >> 8) & 255; break;
            case 4: hb = (size >> 16) & 255; break; case 5: hb = (size >> 24) & 255; break;
            case 10: hb = 0x1A; break; case 14: hb = 12; break;
            case 18: hb = im.width & 255; break; case 19: hb = (im.width >> 8) & 255; break;
            case 20: hb = im.height & 255; break; case 21: hb = (im.height >> 8) & 255; break;
            case 22: hb = 1; break; case 24: hb = 24; break;
            default: hb = 0;
        }
        out[tid] = hb;
    }
    // Colour + store: a thread takes FOUR horizontally adjacent pixels (12 output bytes, written as one
    // 12-byte store -- gfx950 global stores need no alignment), thread rows of 64 items sweep `mh` picture
    // rows four at a time.  No runtime divisions: mw is 8 or 16, the MCU grid position was tabulated once.
    const uint32_t q_log = hs == 2 ? 2u : 1u;                  // log2(mw / 4): items per MCU row
    const uint32_t hs_log = hs - 1, vs_log = vs - 1;
    const uint32_t items = wg.n_mcu << q_log;
    struct __attribute__((packed)) Px12 { uint32_t a, b, c; };
    // item (MCU, 4-pixel column group) outside, picture row inside: everything that depends only on the item
    // (grid position, X, the unit indices) is computed once per item instead of once per row
    for (uint32_t it = tid & 63; it < items; it += 64) {
        const uint32_t ml = it >> q_log, px0 = (it & ((1u << q_log) - 1)) * 4;
        const uint32_t xy = mcu_xy[ml];
        const uint32_t X = __umul24(xy & 0xffffu, mw) + px0, Y0 = __umul24(xy >> 16, mh);
        if (X >= width) continue;
        const uint32_t d0 = __umul24(ml, dus);
        for (uint32_t py = tid >> 6; py < mh; py += PJD_IDCT_THREADS / 64) {
            const uint32_t cy = py >> vs_log, lrow = (py >> 3) * hs, yoff = (py & 7) * 8;
            const uint32_t Y = Y0 + py;
            if (Y >= height) continue;
            const int16_t *yp = &tile[d0 + lrow + (px0 >> 3)][yoff + (px0 & 7)];
            const uint2 yraw = *reinterpret_cast<const uint2 *>(yp);               // 4 luma samples
            const int y0 = (int16_t)(yraw.x & 0xffff), y1 = (int16_t)(yraw.x >> 16), y2 = (int16_t)(yraw.y & 0xffff), y3 = (int16_t)(yraw.y >> 16);
            // chroma terms of pjd_ycc_to_rgb, once per chroma SAMPLE (two pixels share one when hs == 2), already
            // ordered first / middle / last output byte (R,G,B -- or B,G,R for the BMP image) and with the +128
            const uint32_t q = cy * 8 + (px0 >> hs_log);
            int cf[4], cg[4], cl[4];
            const int n_chroma = hs == 2 ? 2 : 4;
            uint2 cbw = make_uint2(0, 0), crw = make_uint2(0, 0);
            if (nc > 1) { if (hs == 2) cbw.x = *reinterpret_cast<const uint32_t *>(&tile[d0 + nl][q]); else cbw = *reinterpret_cast<const uint2 *>(&tile[d0 + nl][q]); }
            if (nc > 2) { if (hs == 2) crw.x = *reinterpret_cast<const uint32_t *>(&tile[d0 + nl + 1][q]); else crw = *reinterpret_cast<const uint2 *>(&tile[d0 + nl + 1][q]); }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j < n_chroma) {
                    const uint32_t bw = j < 2 ? cbw.x : cbw.y, rw = j < 2 ? crw.x : crw.y;
                    const int cbv = (j & 1) ? (int)(int16_t)(bw >> 16) : (int)(int16_t)(bw & 0xffff);
                    const int crv = (j & 1) ? (int)(int16_t)(rw >> 16) : (int)(int16_t)(rw & 0xffff);
                    const int rC = (__mul24(5880414, crv) >> 22) + 128, bC = (__mul24(7432306, cbv) >> 22) + 128;
                    cg[j] = 128 - (__mul24(1442840, cbv) >> 22) - (__mul24(2994733, crv) >> 22);
                    cf[j] = bmp ? bC : rC;
                    cl[j] = bmp ? rC : bC;
                }
            }
            const int s1 = hs == 2 ? 0 : 1, s2 = hs == 2 ? 1 : 2, s3 = hs == 2 ? 1 : 3;   // chroma sample of pixels 1..3
            const int cf1 = s1 ? cf[1] : cf[0], cg1 = s1 ? cg[1] : cg[0], cl1 = s1 ? cl[1] : cl[0];
            const int cf2 = s2 == 2 ? cf[2] : cf[1], cg2 = s2 == 2 ? cg[2] : cg[1], cl2 = s2 == 2 ? cl[2] : cl[1];
            const int cf3 = s3 == 3 ? cf[3] : cf[1], cg3 = s3 == 3 ? cg[3] : cg[1], cl3 = s3 == 3 ? cl[3] : cl[1];
            // reference src/decoder_dpu.c:376-382: y + term + 128, clamped
            const uint32_t f0 = pjd_clamp255(y0 + cf[0]), g0 = pjd_clamp255(y0 + cg[0]), l0 = pjd_clamp255(y0 + cl[0]);
            const uint32_t f1 = pjd_clamp255(y1 + cf1), g1 = pjd_clamp255(y1 + cg1), l1 = pjd_clamp255(y1 + cl1);
            const uint32_t f2 = pjd_clamp255(y2 + cf2), g2 = pjd_clamp255(y2 + cg2), l2 = pjd_clamp255(y2 + cl2);
            const uint32_t f3 = pjd_clamp255(y3 + cf3), g3 = pjd_clamp255(y3 + cg3), l3 = pjd_clamp255(y3 + cl3);
            if (PLANAR) {
                // three plane rows (stride = width, plane = width x height); first / middle / last are R, G, B here
                const size_t plane = (size_t)stride * height;
                uint8_t *o = out + (size_t)Y * stride + X;
                if (X + 4 <= width) {
                    reinterpret_cast<PjdPx4 *>(o)->a = f0 | (f1 << 8) | (f2 << 16) | (f3 << 24);
                    reinterpret_cast<PjdPx4 *>(o + plane)->a = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
                    reinterpret_cast<PjdPx4 *>(o + 2 * plane)->a = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
                } else {                                                         // right picture edge
                    o[0] = (uint8_t)f0; o[plane] = (uint8_t)g0; o[2 * plane] = (uint8_t)l0;
                    if (X + 1 < width) { o[1] = (uint8_t)f1; o[plane + 1] = (uint8_t)g1; o[2 * plane + 1] = (uint8_t)l1; }
                    if (X + 2 < width) { o[2] = (uint8_t)f2; o[plane + 2] = (uint8_t)g2; o[2 * plane + 2] = (uint8_t)l2; }
                }
                continue;
            }
            uint8_t *o = bmp ? out + 26 + (size_t)(height - 1 - Y) * stride + X * 3
                             : out + (size_t)Y * stride + X * 3;
            if (X + 4 <= width) {
                Px12 v;
                v.a = f0 | (g0 << 8) | (l0 << 16) | (f1 << 24);
                v.b = g1 | (l1 << 8) | (f2 << 16) | (g2 << 24);
                v.c = l2 | (f3 << 8) | (g3 << 16) | (l3 << 24);
                *reinterpret_cast<Px12 *>(o) = v;
            } else {                                                             // right picture edge
                o[0] = (uint8_t)f0; o[1] = (uint8_t)g0; o[2] = (uint8_t)l0;
                if (X + 1 < width) { o[3] = (uint8_t)f1; o[4] = (uint8_t)g1; o[5] = (uint8_t)l1; }
                if (X + 2 < width) { o[6] = (uint8_t)f2; o[7] = (uint8_t)g2; o[8] = (uint8_t)l2; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Chroma upsample + colour + raster store, specialised by sampling mode and output format (the generic version is
// the tail of pjd_tile_to_pixels).  A thread takes a block of 4 x VS pixels: the VS picture rows share their chroma
// samples (nearest neighbour, reference src/decoder_dpu.c:370), so the chroma terms of the conversion
// (reference src/decoder_dpu.c:376-382) are computed once per sample.  A wave sweeps one row group across all MCUs of
// the workgroup: its stores cover whole runs of a picture row.
// ---------------------------------------------------------------------------------------------

// PLANAR (never with BMP): three 4-byte stores, one per plane, instead of the 12-byte store; `stride` is the plane row (= width) and
// `plane` the bytes of a plane.  A wave's store instruction then covers runs of one plane row, a dword per lane.
template <int HS, int VS, bool BMP, bool PLANAR = false>
__device__ __forceinline__ void pjd_colour_store(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, uint8_t *out,
                                                 uint32_t width, uint32_t height, uint32_t stride, uint32_t ncomp,
                                                 uint32_t n_mcu, uint32_t tid, size_t plane = 0)
{
    static_assert(!(BMP && PLANAR), "a BMP file image is interleaved");
    constexpr uint32_t MW = 8 * HS, MH = 8 * VS, NL = HS * VS;
    constexpr uint32_t CG_LOG = HS == 2 ? 2 : 1;               // log2 of the 4-pixel column groups per MCU row
    constexpr int NCH = 4 / HS;                                 // chroma samples under 4 pixels
    const uint32_t dus = NL + ncomp - 1;
    const uint32_t per_row = n_mcu << CG_LOG;
    const uint32_t lane = tid & 63, wv = tid >> 6;
    for (uint32_t rg = wv; rg < 8; rg += PJD_IDCT_THREADS / 64) {          // row group = VS picture rows = one chroma row
        for (uint32_t idx = lane; idx < per_row; idx += 64) {
            const uint32_t ml = idx >> CG_LOG, px0 = (idx & ((1u << CG_LOG) - 1)) * 4;
            const uint32_t xy = mcu_xy[ml];
            const uint32_t X = __umul24(xy & 0xffffu, MW) + px0, Y0 = __umul24(xy >> 16, MH) + rg * VS;
            if (X >= width || Y0 >= height) continue;
            const uint32_t d0 = __umul24(ml, dus);
            // chroma terms, ordered first / middle / last output byte (R,G,B -- or B,G,R for the BMP image), +128 included
            int cf[NCH], cg[NCH], cl[NCH];
            bool fast = X + 4 <= width;
            {
                const uint32_t q = rg * 8 + px0 / HS;
                uint32_t cbw[2] = {0, 0}, crw[2] = {0, 0};
                if (ncomp > 1) {
                    if (HS == 2) cbw[0] = *reinterpret_cast<const uint32_t *>(&tile[d0 + NL][q]);
                    else { const uint2 t = *reinterpret_cast<const uint2 *>(&tile[d0 + NL][q]); cbw[0] = t.x; cbw[1] = t.y; }
                }
                if (ncomp > 2) {
                    if (HS == 2) crw[0] = *reinterpret_cast<const uint32_t *>(&tile[d0 + NL + 1][q]);
                    else { const uint2 t = *reinterpret_cast<const uint2 *>(&tile[d0 + NL + 1][q]); crw[0] = t.x; crw[1] = t.y; }
                }
                // the packed rows below need every chroma term in int16: all chroma samples under the task in [-16384, 16383]
                uint32_t oor = pjd_chroma_out_of_range(cbw[0]) | pjd_chroma_out_of_range(crw[0]);
                if (HS == 1) oor |= pjd_chroma_out_of_range(cbw[1]) | pjd_chroma_out_of_range(crw[1]);
                fast = fast && oor == 0;
#pragma unroll
                for (int j = 0; j < NCH; j++) {
                    const uint32_t bw = cbw[j >> 1], rw = crw[j >> 1];
                    const int cbv = (j & 1) ? (int)bw >> 16 : (int)(int16_t)(bw & 0xffff);
                    const int crv = (j & 1) ? (int)rw >> 16 : (int)(int16_t)(rw & 0xffff);
                    const int rC = (__mul24(5880414, crv) >> 22) + 128, bC = (__mul24(7432306, cbv) >> 22) + 128;
                    cg[j] = 128 - (__mul24(1442840, cbv) >> 22) - (__mul24(2994733, crv) >> 22);
                    cf[j] = BMP ? bC : rC;
                    cl[j] = BMP ? rC : bC;
                }
            }
            if (fast) {
                // Packed rows: the luma samples lie in LDS as two int16 pairs; pair + chroma-term pair with signed saturation, then
                // saturation to bytes -- equal to pjd_clamp255(y + term) (pjd_device_common.h).  The term pairs serve all VS rows.
                constexpr int s1 = HS == 2 ? 0 : 1, s2 = HS == 2 ? 1 : 2, s3 = HS == 2 ? 1 : 3;   // chroma sample of pixels 1..3
                const uint32_t pf01 = pjd_pack_i16(cf[0], cf[s1]), pf23 = pjd_pack_i16(cf[s2], cf[s3]);
                const uint32_t pg01 = pjd_pack_i16(cg[0], cg[s1]), pg23 = pjd_pack_i16(cg[s2], cg[s3]);
                const uint32_t pl01 = pjd_pack_i16(cl[0], cl[s1]), pl23 = pjd_pack_i16(cl[s2], cl[s3]);
#pragma unroll
                for (int v = 0; v < VS; v++) {
                    const uint32_t Y = Y0 + v;
                    if (Y >= height) break;
                    const uint32_t py = rg * VS + v;
                    const int16_t *yp = &tile[d0 + (py >> 3) * HS + (px0 >> 3)][(py & 7) * 8 + (px0 & 7)];
                    const uint2 yraw = *reinterpret_cast<const uint2 *>(yp);               // 4 luma samples: (y0, y1), (y2, y3)
                    const uint32_t f01 = pjd_pk_add_i16_sat(yraw.x, pf01), f23 = pjd_pk_add_i16_sat(yraw.y, pf23);
                    const uint32_t g01 = pjd_pk_add_i16_sat(yraw.x, pg01), g23 = pjd_pk_add_i16_sat(yraw.y, pg23);
                    const uint32_t l01 = pjd_pk_add_i16_sat(yraw.x, pl01), l23 = pjd_pk_add_i16_sat(yraw.y, pl23);
                    if (PLANAR) {
                        uint32_t f = pjd_sat_pk_u8_i16(f01), g = pjd_sat_pk_u8_i16(g01), l = pjd_sat_pk_u8_i16(l01);
                        pjd_sat_pk_u8_i16_hi(f, f23); pjd_sat_pk_u8_i16_hi(g, g23); pjd_sat_pk_u8_i16_hi(l, l23);
                        uint8_t *o = out + (size_t)Y * stride + X;
                        reinterpret_cast<PjdPx4 *>(o)->a = f;
                        reinterpret_cast<PjdPx4 *>(o + plane)->a = g;
                        reinterpret_cast<PjdPx4 *>(o + 2 * plane)->a = l;
                    } else {
                        // p = f0 f1 l0 l1, m = g0 g1 g2 g3, r = f2 f3 l2 l3: each of the three output dwords takes bytes of two of them,
                        // but for the middle one (g1 l1 f2 g2), which takes two steps
                        uint32_t p = pjd_sat_pk_u8_i16(f01), m = pjd_sat_pk_u8_i16(g01), r = pjd_sat_pk_u8_i16(f23);
                        pjd_sat_pk_u8_i16_hi(p, l01); pjd_sat_pk_u8_i16_hi(m, g23); pjd_sat_pk_u8_i16_hi(r, l23);
                        PjdPx12 px;
                        px.a = pjd_perm(m, p, 0x01020400u);                                // f0 g0 l0 f1
                        px.b = pjd_perm(m, pjd_perm(p, r, 0x00000700u), 0x06020105u);      // (f2 l1 f2 f2) -> g1 l1 f2 g2
                        px.c = pjd_perm(m, r, 0x03070102u);                                // l2 f3 g3 l3
                        uint8_t *o = BMP ? out + 26 + (size_t)(height - 1 - Y) * stride + X * 3 : out + (size_t)Y * stride + X * 3;
                        *reinterpret_cast<PjdPx12 *>(o) = px;
                    }
                }
                continue;
            }
            // the right picture edge inside the 4 pixels, or a chroma sample outside that range: 32-bit sums, a clamp per byte
#pragma unroll
            for (int v = 0; v < VS; v++) {
                const uint32_t Y = Y0 + v;
                if (Y >= height) break;
                const uint32_t py = rg * VS + v;
                const int16_t *yp = &tile[d0 + (py >> 3) * HS + (px0 >> 3)][(py & 7) * 8 + (px0 & 7)];
                const uint2 yraw = *reinterpret_cast<const uint2 *>(yp);               // 4 luma samples
                const int y0 = (int16_t)(yraw.x & 0xffff), y1 = (int)yraw.x >> 16, y2 = (int16_t)(yraw.y & 0xffff), y3 = (int)yraw.y >> 16;
                constexpr int s1 = HS == 2 ? 0 : 1, s2 = HS == 2 ? 1 : 2, s3 = HS == 2 ? 1 : 3;   // chroma sample of pixels 1..3
                const uint32_t f0 = pjd_clamp255(y0 + cf[0]), g0 = pjd_clamp255(y0 + cg[0]), l0 = pjd_clamp255(y0 + cl[0]);
                const uint32_t f1 = pjd_clamp255(y1 + cf[s1]), g1 = pjd_clamp255(y1 + cg[s1]), l1 = pjd_clamp255(y1 + cl[s1]);
                const uint32_t f2 = pjd_clamp255(y2 + cf[s2]), g2 = pjd_clamp255(y2 + cg[s2]), l2 = pjd_clamp255(y2 + cl[s2]);
                const uint32_t f3 = pjd_clamp255(y3 + cf[s3]), g3 = pjd_clamp255(y3 + cg[s3]), l3 = pjd_clamp255(y3 + cl[s3]);
                if (PLANAR) {
                    uint8_t *o = out + (size_t)Y * stride + X;
                    if (X + 4 <= width) {
                        reinterpret_cast<PjdPx4 *>(o)->a = f0 | (f1 << 8) | (f2 << 16) | (f3 << 24);
                        reinterpret_cast<PjdPx4 *>(o + plane)->a = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
                        reinterpret_cast<PjdPx4 *>(o + 2 * plane)->a = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
                    } else {                                                         // right picture edge
                        o[0] = (uint8_t)f0; o[plane] = (uint8_t)g0; o[2 * plane] = (uint8_t)l0;
                        if (X + 1 < width) { o[1] = (uint8_t)f1; o[plane + 1] = (uint8_t)g1; o[2 * plane + 1] = (uint8_t)l1; }
                        if (X + 2 < width) { o[2] = (uint8_t)f2; o[plane + 2] = (uint8_t)g2; o[2 * plane + 2] = (uint8_t)l2; }
                    }
                    continue;
                }
                uint8_t *o = BMP ? out + 26 + (size_t)(height - 1 - Y) * stride + X * 3 : out + (size_t)Y * stride + X * 3;
                if (X + 4 <= width) {
                    PjdPx12 px;
                    px.a = f0 | (g0 << 8) | (l0 << 16) | (f1 << 24);
                    px.b = g1 | (l1 << 8) | (f2 << 16) | (g2 << 24);
                    px.c = l2 | (f3 << 8) | (g3 << 16) | (l3 << 24);
                    *reinterpret_cast<PjdPx12 *>(o) = px;
                } else {                                                             // right picture edge
                    o[0] = (uint8_t)f0; o[1] = (uint8_t)g0; o[2] = (uint8_t)l0;
                    if (X + 1 < width) { o[3] = (uint8_t)f1; o[4] = (uint8_t)g1; o[5] = (uint8_t)l1; }
                    if (X + 2 < width) { o[6] = (uint8_t)f2; o[7] = (uint8_t)g2; o[8] = (uint8_t)l2; }
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Reduced-size output (PJD_F_SCALE_*, include/pjd.h): output pixel (i, j) is the rounded mean of the clamped 8-bit colours of the
// source box [S*i, S*i + S) x [S*j, S*j + S), cut at the right and bottom picture edge.  S divides 8 and an MCU is 8 or 16 pixels
// on a side, so every box lies inside one MCU of the workgroup.  The colour arithmetic is pjd_colour_store's; a thread takes one
// 4-pixel column group of an MCU over the S picture rows of one box row (the task index runs over all threads of the workgroup)
// and keeps the sums in registers: 4 / S output pixels for S <= 4; at S = 8 the two column groups of a box are neighbouring lanes
// and add their sums with one cross-lane move.  A full box divides by a shift, only edge boxes by n < S * S.
// ---------------------------------------------------------------------------------------------
template <int HS, int VS, bool BMP, int S, bool PLANAR = false>
__device__ __forceinline__ void pjd_colour_store_scaled(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, uint8_t *out,
                                                        uint32_t width, uint32_t height, uint32_t stride, uint32_t ncomp,
                                                        uint32_t n_mcu, uint32_t tid)
{
    static_assert(!(BMP && PLANAR), "a BMP file image is interleaved");
    constexpr uint32_t MW = 8 * HS, MH = 8 * VS, NL = HS * VS;
    constexpr uint32_t CG_LOG = HS == 2 ? 2 : 1;               // log2 of the 4-pixel column groups per MCU row
    constexpr uint32_t S_LOG = S == 2 ? 1 : (S == 4 ? 2 : 3);
    constexpr uint32_t BR_LOG = (VS == 2 ? 4 : 3) - S_LOG;     // log2 of the box rows per MCU (MH / S)
    constexpr int NCH = 4 / HS;                                 // chroma samples under 4 pixels
    constexpr int NO = S < 4 ? 4 / S : 1;                       // output pixels a thread sums for
    constexpr int PX_LOG = S < 4 ? S_LOG : 2;                   // log2 of the pixels of a row that go into one of them
    static_assert(MH % S == 0 && S % VS == 0, "a box lies inside one MCU and covers whole chroma rows");
    const uint32_t dus = NL + ncomp - 1;
    const uint32_t tasks = n_mcu << (CG_LOG + BR_LOG);          // even: the two halves of an 8-wide box run in the same iterations
    const uint32_t sh = (height + S - 1) >> S_LOG;
    for (uint32_t t = tid; t < tasks; t += PJD_IDCT_THREADS) {
        const uint32_t ml = t >> (CG_LOG + BR_LOG), j = (t >> CG_LOG) & ((1u << BR_LOG) - 1), px0 = (t & ((1u << CG_LOG) - 1)) * 4;
        const uint32_t xy = mcu_xy[ml];
        const uint32_t X = __umul24(xy & 0xffffu, MW) + px0, Yb = __umul24(xy >> 16, MH) + j * S;   // first pixel, first row of the box
        const uint32_t d0 = __umul24(ml, dus);
        uint32_t sf[NO], sg[NO], sl[NO];                        // sums of the first / middle / last output byte
#pragma unroll
        for (int k = 0; k < NO; k++) sf[k] = sg[k] = sl[k] = 0;
        if (X < width && Yb < height) {
#pragma unroll
            for (uint32_t k = 0; k < S / VS; k++) {             // the chroma rows (row groups) of the box row
                const uint32_t rg = j * (S / VS) + k, Y0 = Yb + k * VS;
                if (Y0 >= height) break;
                int cf[NCH], cg[NCH], cl[NCH];
                {
                    const uint32_t q = rg * 8 + px0 / HS;
                    uint32_t cbw[2] = {0, 0}, crw[2] = {0, 0};
                    if (ncomp > 1) {
                        if (HS == 2) cbw[0] = *reinterpret_cast<const uint32_t *>(&tile[d0 + NL][q]);
                        else { const uint2 t2 = *reinterpret_cast<const uint2 *>(&tile[d0 + NL][q]); cbw[0] = t2.x; cbw[1] = t2.y; }
                    }
                    if (ncomp > 2) {
                        if (HS == 2) crw[0] = *reinterpret_cast<const uint32_t *>(&tile[d0 + NL + 1][q]);
                        else { const uint2 t2 = *reinterpret_cast<const uint2 *>(&tile[d0 + NL + 1][q]); crw[0] = t2.x; crw[1] = t2.y; }
                    }
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        const uint32_t bw = cbw[c >> 1], rw = crw[c >> 1];
                        const int cbv = (c & 1) ? (int)bw >> 16 : (int)(int16_t)(bw & 0xffff);
                        const int crv = (c & 1) ? (int)rw >> 16 : (int)(int16_t)(rw & 0xffff);
                        const int rC = (__mul24(5880414, crv) >> 22) + 128, bC = (__mul24(7432306, cbv) >> 22) + 128;
                        cg[c] = 128 - (__mul24(1442840, cbv) >> 22) - (__mul24(2994733, crv) >> 22);
                        cf[c] = BMP ? bC : rC;
                        cl[c] = BMP ? rC : bC;
                    }
                }
#pragma unroll
                for (int v = 0; v < VS; v++) {
                    if (Y0 + v >= height) break;
                    const uint32_t py = rg * VS + v;
                    const int16_t *yp = &tile[d0 + (py >> 3) * HS + (px0 >> 3)][(py & 7) * 8 + (px0 & 7)];
                    const uint2 yraw = *reinterpret_cast<const uint2 *>(yp);               // 4 luma samples
                    const int yv[4] = {(int16_t)(yraw.x & 0xffff), (int)yraw.x >> 16, (int16_t)(yraw.y & 0xffff), (int)yraw.y >> 16};
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const int c = HS == 2 ? p >> 1 : p;                                  // chroma sample of pixel p
                        // reference src/decoder_dpu.c:376-382: y + term + 128, clamped; pixels past the right edge do not count
                        const bool in = p == 0 || X + p < width;
                        sf[p >> PX_LOG] += in ? (uint32_t)pjd_clamp255(yv[p] + cf[c]) : 0u;
                        sg[p >> PX_LOG] += in ? (uint32_t)pjd_clamp255(yv[p] + cg[c]) : 0u;
                        sl[p >> PX_LOG] += in ? (uint32_t)pjd_clamp255(yv[p] + cl[c]) : 0u;
                    }
                }
            }
        }
        if (S == 8) {                                           // the other half of the box: lane t ^ 1 (t and the lane index share bit 0)
            sf[0] += (uint32_t)__shfl_xor((int)sf[0], 1);
            sg[0] += (uint32_t)__shfl_xor((int)sg[0], 1);
            sl[0] += (uint32_t)__shfl_xor((int)sl[0], 1);
        }
        if (X < width && Yb < height && (S < 8 || (px0 & 4) == 0)) {
            const uint32_t bh = height - Yb < S ? height - Yb : S;
            const uint32_t oy = Yb >> S_LOG, ox = X >> S_LOG;
            const size_t plane = PLANAR ? (size_t)stride * sh : 0;                 // PLANAR: stride is the plane row, ceil(width / S)
            uint8_t *o = PLANAR ? out + (size_t)oy * stride + ox
                                : (BMP ? out + 26 + (size_t)(sh - 1 - oy) * stride + ox * 3 : out + (size_t)oy * stride + ox * 3);
#pragma unroll
            for (int k = 0; k < NO; k++) {
                const uint32_t bx = X + k * S;                  // first column of the box
                if (k > 0 && bx >= width) break;
                const uint32_t n = (width - bx < S ? width - bx : S) * bh;
                uint32_t a, b, c;
                if (n == S * S) { a = (sf[k] + S * S / 2) >> (2 * S_LOG); b = (sg[k] + S * S / 2) >> (2 * S_LOG); c = (sl[k] + S * S / 2) >> (2 * S_LOG); }
                else { a = (sf[k] + (n >> 1)) / n; b = (sg[k] + (n >> 1)) / n; c = (sl[k] + (n >> 1)) / n; }
                if (PLANAR) { o[k] = (uint8_t)a; o[plane + k] = (uint8_t)b; o[2 * plane + k] = (uint8_t)c; }
                else { o[3 * k] = (uint8_t)a; o[3 * k + 1] = (uint8_t)b; o[3 * k + 2] = (uint8_t)c; }
            }
        }
    }
}

template <bool PLANAR>
__device__ __forceinline__ void pjd_colour_dispatch_scaled(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, const PjdDevBatch &B,
                                                           const PjdDevImage &im, const PjdDevIdctWg &wg, uint32_t tid)
{
    uint8_t *out = B.out + im.out_off;
    const uint32_t width = im.width, height = im.height, stride = im.out_stride, nc = im.ncomp, n = wg.n_mcu;
    if (PLANAR) {
        const uint32_t mode = (im.hs - 1) | ((im.vs - 1) << 1) | ((((im.flags & PJD_IF_SCALE_MASK) >> PJD_IF_SCALE_SHIFT) - 1) << 2);
#define PJD_PLANAR_CASES(M0, S_)                                                                                                  \
    case M0 + 0: pjd_colour_store_scaled<1, 1, false, S_, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;     \
    case M0 + 1: pjd_colour_store_scaled<2, 1, false, S_, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;     \
    case M0 + 2: pjd_colour_store_scaled<1, 2, false, S_, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;     \
    case M0 + 3: pjd_colour_store_scaled<2, 2, false, S_, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        switch (mode) {
            PJD_PLANAR_CASES(0, 2)
            PJD_PLANAR_CASES(4, 4)
            PJD_PLANAR_CASES(8, 8)
            default: break;
        }
#undef PJD_PLANAR_CASES
        return;
    }
    const bool bmp = (im.flags & PJD_IF_BMP) != 0;
    const uint32_t s_log = (im.flags & PJD_IF_SCALE_MASK) >> PJD_IF_SCALE_SHIFT;          // 1..3
    if (bmp && wg.first_mcu == 0) pjd_bmp_header(out, (width + (1u << s_log) - 1) >> s_log, (height + (1u << s_log) - 1) >> s_log, stride, tid);
    const uint32_t mode = (im.hs - 1) | ((im.vs - 1) << 1) | (bmp ? 4u : 0u) | ((s_log - 1) << 3);
#define PJD_SCALED_CASE(M, HS_, VS_, BMP_, S_) \
    case M: pjd_colour_store_scaled<HS_, VS_, BMP_, S_>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
#define PJD_SCALED_CASES(M0, S_)                                                                                          \
    PJD_SCALED_CASE(M0 + 0, 1, 1, false, S_) PJD_SCALED_CASE(M0 + 1, 2, 1, false, S_) PJD_SCALED_CASE(M0 + 2, 1, 2, false, S_) \
    PJD_SCALED_CASE(M0 + 3, 2, 2, false, S_) PJD_SCALED_CASE(M0 + 4, 1, 1, true, S_)  PJD_SCALED_CASE(M0 + 5, 2, 1, true, S_)  \
    PJD_SCALED_CASE(M0 + 6, 1, 2, true, S_)  PJD_SCALED_CASE(M0 + 7, 2, 2, true, S_)
    switch (mode) {
        PJD_SCALED_CASES(0, 2)
        PJD_SCALED_CASES(8, 4)
        PJD_SCALED_CASES(16, 8)
        default: break;
    }
#undef PJD_SCALED_CASES
#undef PJD_SCALED_CASE
}

// SCALED: the kernel also serves pictures with an output scale (a kernel of its own, so that the full-size kernels stay as they are)
template <bool SCALED, bool PLANAR = false>
__device__ __forceinline__ void pjd_colour_dispatch(const int16_t (*tile)[TILE_STRIDE], const uint32_t *mcu_xy, const PjdDevBatch &B,
                                                    const PjdDevImage &im, const PjdDevIdctWg &wg, uint32_t tid)
{
    if (SCALED && (im.flags & PJD_IF_SCALE_MASK)) { pjd_colour_dispatch_scaled<PLANAR>(tile, mcu_xy, B, im, wg, tid); return; }
    uint8_t *out = B.out + im.out_off;
    const uint32_t width = im.width, height = im.height, stride = im.out_stride, nc = im.ncomp, n = wg.n_mcu;
    if (PLANAR) {
        const size_t plane = (size_t)stride * height;          // computed once per workgroup: no division anywhere near a store
        switch ((im.hs - 1) | ((im.vs - 1) << 1)) {
            case 0: pjd_colour_store<1, 1, false, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid, plane); break;
            case 1: pjd_colour_store<2, 1, false, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid, plane); break;
            case 2: pjd_colour_store<1, 2, false, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid, plane); break;
            default: pjd_colour_store<2, 2, false, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid, plane); break;
        }
        return;
    }
    const bool bmp = (im.flags & PJD_IF_BMP) != 0;
    if (bmp && wg.first_mcu == 0) pjd_bmp_header(out, width, height, stride, tid);
    const uint32_t mode = (im.hs - 1) | ((im.vs - 1) << 1) | (bmp ? 4u : 0u);
    switch (mode) {
        case 0: pjd_colour_store<1, 1, false>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 1: pjd_colour_store<2, 1, false>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 2: pjd_colour_store<1, 2, false>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 3: pjd_colour_store<2, 2, false>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 4: pjd_colour_store<1, 1, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 5: pjd_colour_store<2, 1, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        case 6: pjd_colour_store<1, 2, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
        default: pjd_colour_store<2, 2, true>(tile, mcu_xy, out, width, height, stride, nc, n, tid); break;
    }
}

// ---------------------------------------------------------------------------------------------
// Fused back end.  One workgroup = up to 96 data units = a run of consecutive MCUs of one image.
// ---------------------------------------------------------------------------------------------
// SCALED: the form for a batch that holds pictures with an output scale (PJD_F_SCALE_*); a kernel of its own, so that the full-size one
// keeps its code and registers
template <bool SCALED>
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_colour(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base)
{
#define PJD_DENSE_PLANAR false
#include "pjd_k_idct_dense_body.h"
#undef PJD_DENSE_PLANAR
}

// The same for a PJD_OUT_RGB8_PLANAR batch: kernels of their own, so that the interleaved ones keep their code and registers
template <bool SCALED>
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_colour_planar(PjdDevBatch B, const PjdDevIdctWg *__restrict__ wgs, const uint64_t *__restrict__ dense_base)
{
#define PJD_DENSE_PLANAR true
#include "pjd_k_idct_dense_body.h"
#undef PJD_DENSE_PLANAR
}

// ---------------------------------------------------------------------------------------------
// Lane-stream front end: the parallel entropy decoder leaves one 16-bit entry per symbol in per-lane
// regions, in 32-byte groups of a head and 14 entries (layout: pjd_internal.h), the data unit every lane starts in, and,
// for the first data unit of every IDCT workgroup, a mark (lane, slot, DC sums so far).  The workgroup finds the lanes its
// range of units lies in, and one thread per group walks the group from its head: unit index and zigzag slot of every
// entry follow from the head and the entries before it in the group; it de-zigzags and dequantises into the LDS tile.
// ---------------------------------------------------------------------------------------------


// One back-end range (PjdDevIdctWg `iwg`) by the whole workgroup; the LDS arrays are the kernel's.  Returns are workgroup-uniform.
// SCALED: pictures with an output scale take the scaled store.  PLANAR: the batch's output format is PJD_OUT_RGB8_PLANAR.
template <bool SCALED, bool PLANAR = false>
__device__ __forceinline__ void pjd_idct_range(const PjdDevBatch &B, uint32_t iwg, int16_t (*tile)[TILE_STRIDE], uint32_t (*qz)[64], uint32_t *mcu_xy,
                                               uint8_t *comp_of, uint8_t *du_head, uint32_t *wagg, uint32_t *ltab)
{
#include "pjd_k_lanes_parse_body.h"
    // ---- DC prediction over the range (reference src/jpeg_scanner.cpp:485-486) by wave 0, while the other waves already do
    //      the row pass of rows 1..7 (only row 0 holds the DC coefficient) and the slot-52 rule (natural 38 lies in row 4)
    if (wv != 0) {
        for (uint32_t i = tid - 64; i < n_du * 7; i += PJD_IDCT_THREADS - 64) {
            const uint32_t u = pjd_div_small(i, c_recip16[7]), r = 1 + (i - __umul24(u, 7u));   // i < 7 * PJD_IDCT_MAX_DU: exact
            if (r == 4 && tile[u][64] != (int16_t)PJD_COEF_SENTINEL) tile[u][38] = (int16_t)pjd_dequant((int)tile[u][64], qz[comp_of[u]][48] & 0xffffu);   // slot 52 over natural 38 (the quantiser of slot 48 is that position's)
            pjd_tile_row(tile, u, r);
        }
    } else {
#include "pjd_k_lanes_dc_body.h"
    }
    // ---- IDCT (reference src/decoder_dpu.c:210-321): rows, then columns; then colour
    __syncthreads();
    for (uint32_t u = tid; u < n_du; u += PJD_IDCT_THREADS) pjd_tile_row(tile, u, 0);
    __syncthreads();
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) pjd_tile_col(tile, i >> 3, i & 7);
    __syncthreads();
    pjd_colour_dispatch<SCALED, PLANAR>(tile, mcu_xy, B, im, wg, tid);
}

// order: the launch's workgroup -> index into PjdDevBatch::iwgs / marks (null: the identity, one launch for the whole batch)
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_colour_lanes(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    PJD_LANES_LDS

#if PJD_IDCT_PRIO
    __builtin_amdgcn_s_setprio(PJD_IDCT_PRIO);
#endif
    pjd_idct_range<false>(B, order ? order[blockIdx.x] : blockIdx.x, tile, qz, mcu_xy, comp_of, du_head, wagg, ltab);
}

// The same for a batch that holds pictures with an output scale (PJD_F_SCALE_*): a kernel of its own, so that the full-size one keeps
// its code and registers.
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_colour_lanes_scaled(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    PJD_LANES_LDS

#if PJD_IDCT_PRIO
    __builtin_amdgcn_s_setprio(PJD_IDCT_PRIO);
#endif
    pjd_idct_range<true>(B, order ? order[blockIdx.x] : blockIdx.x, tile, qz, mcu_xy, comp_of, du_head, wagg, ltab);
}

// The lane-stream back end of a PJD_OUT_RGB8_PLANAR batch, without and with pictures that have an output scale: kernels of their own
// again.
template <bool SCALED>
__global__ __launch_bounds__(PJD_IDCT_THREADS) void pjd_k_idct_colour_lanes_planar(PjdDevBatch B, const uint32_t *__restrict__ order)
{
    PJD_LANES_LDS

#if PJD_IDCT_PRIO
    __builtin_amdgcn_s_setprio(PJD_IDCT_PRIO);
#endif
    pjd_idct_range<SCALED, true>(B, order ? order[blockIdx.x] : blockIdx.x, tile, qz, mcu_xy, comp_of, du_head, wagg, ltab);
}

// The kernel of a form for lane-stream input.
void pjd_launch_idct_lanes(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const uint32_t *order, uint32_t n_wg)
{
    if (n_wg == 0) return;
    if (f.layout == PJD_BACK_INTERLEAVED && !f.scaled) {
        hipLaunchKernelGGL(pjd_k_idct_colour_lanes, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, order);
        return;
    }
    // scaled before full size in every table of the back end: the order the templates are instantiated in is part of a unit's text
    static const PjdLanesKernel colour[3] = {pjd_k_idct_colour_lanes_planar<true>, pjd_k_idct_colour_lanes_planar<false>, pjd_k_idct_colour_lanes_scaled};
    const PjdLanesKernel k = f.gray() ? pjd_gray_lanes_kernel(f.scaled ? PJD_GRAY_SCALED : PJD_GRAY_FULL) : colour[f.layout == PJD_BACK_PLANAR ? !f.scaled : 2];
    hipLaunchKernelGGL(k, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, order);
}

// ---------------------------------------------------------------------------------------------
// One picture group: verdict and DC predictors per PICTURE, one workgroup each (pictures of a group are small: the planner makes
// groups only if no picture has more than 8192 lanes).  The same results as pjd_k_image_verdict + pjd_k_lane_dc_local / _carry leave,
// with every lane's predictors absolute (PjdDevLaneDc::abs = 1: no block carry to add).
// images == null: workgroup k takes picture k -- the whole batch in the single chain (PjdPlan::dc_per_picture); a picture routed to
// the exact kernel up front has no lanes and keeps its status word.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJD_DC_BLOCK) void pjd_k_group_dc(PjdDevBatch B, const uint32_t *__restrict__ images)
{
    __shared__ uint32_t sy[PJD_DC_BLOCK], scb[PJD_DC_BLOCK], scr[PJD_DC_BLOCK], sf[PJD_DC_BLOCK];
    const uint32_t i = images ? images[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
    const PjdDevImage &im = B.images[i];
    if (tid == 0) {                                            // pjd_k_image_verdict
        const int32_t st = B.status[i];
        if (!(st & PJD_STW_NEEDS_EXACT)) {
            const PjdDevImState s = B.imstate[i];
            const bool has_err = s.err_key != ~0ull;
            const uint32_t err_pos = (uint32_t)(s.err_key >> 32);
            const bool flagged = s.flag_pos != 0xffffffffu && s.flag_pos <= s.end_pos;
            if (flagged && (!has_err || s.flag_pos <= err_pos)) B.status[i] = st | PJD_STW_NEEDS_EXACT;
            else if (has_err) B.status[i] = (int32_t)((s.err_key >> 1) & 7u);
        }
    }
    uint32_t cy = 0, ccb = 0, ccr = 0;                         // predictors entering the current chunk of lanes
    for (uint32_t base = 0; base < im.n_lane; base += PJD_DC_BLOCK) {
        const uint32_t q = im.lane_base + base + tid;
        const bool on = base + tid < im.n_lane;
        uint32_t vy = 0, vcb = 0, vcr = 0, head = 0;
        if (on) {
            const PjdDevLaneInfo li = B.lane_info[q];
            vy = li.dc_sum[0]; vcb = li.dc_sum[1]; vcr = li.dc_sum[2]; head = li.first_du >> 31;
        }
        sy[tid] = vy; scb[tid] = vcb; scr[tid] = vcr; sf[tid] = head;
        __syncthreads();
        for (uint32_t off = 1; off < PJD_DC_BLOCK; off <<= 1) {      // Hillis-Steele inclusive segmented scan
            uint32_t ay = 0, acb = 0, acr = 0, af = 0;
            const bool take = tid >= off;
            if (take) { ay = sy[tid - off]; acb = scb[tid - off]; acr = scr[tid - off]; af = sf[tid - off]; }
            const uint32_t myf = sf[tid];
            __syncthreads();
            if (take) {
                if (!myf) { sy[tid] += ay; scb[tid] += acb; scr[tid] += acr; }
                sf[tid] = myf | af;
            }
            __syncthreads();
        }
        if (on) {
            // predictors entering this lane: zero at a segment head; else what the lanes before it leave -- inside the chunk, plus the
            // chunk's carry-in unless a head lies between the chunk start and this lane
            PjdDevLaneDc d;
            d.dc_in[0] = d.dc_in[1] = d.dc_in[2] = 0;
            d.abs = 1;
            if (!head) {
                uint32_t py = cy, pcb = ccb, pcr = ccr;
                if (tid > 0) {
                    const bool h = sf[tid - 1] != 0;
                    py = (h ? 0u : cy) + sy[tid - 1]; pcb = (h ? 0u : ccb) + scb[tid - 1]; pcr = (h ? 0u : ccr) + scr[tid - 1];
                }
                d.dc_in[0] = (uint16_t)py; d.dc_in[1] = (uint16_t)pcb; d.dc_in[2] = (uint16_t)pcr;
            }
            B.lane_dc[q] = d;
        }
        const bool h = sf[PJD_DC_BLOCK - 1] != 0;
        const uint32_t ny = (h ? 0u : cy) + sy[PJD_DC_BLOCK - 1], ncb = (h ? 0u : ccb) + scb[PJD_DC_BLOCK - 1], ncr = (h ? 0u : ccr) + scr[PJD_DC_BLOCK - 1];
        __syncthreads();
        cy = ny; ccb = ncb; ccr = ncr;
    }
}

void pjd_launch_group_dc(hipStream_t s, const PjdDevBatch &b, const PjdDevGroup &g)
{
    if (g.img_count) hipLaunchKernelGGL(pjd_k_group_dc, dim3(g.img_count), dim3(PJD_DC_BLOCK), 0, s, b, b.group_images + g.img_first);
}

void pjd_launch_lane_dc_scan(hipStream_t s, const PjdDevBatch &b, bool per_picture)
{
    if (b.n_dcblk == 0) return;
    if (per_picture) { hipLaunchKernelGGL(pjd_k_group_dc, dim3(b.n_images), dim3(PJD_DC_BLOCK), 0, s, b, (const uint32_t *)nullptr); return; }
    hipLaunchKernelGGL(pjd_k_image_verdict, dim3((b.n_images + 255) / 256), dim3(256), 0, s, b);
    hipLaunchKernelGGL(pjd_k_lane_dc_local, dim3(b.n_dcblk), dim3(PJD_DC_BLOCK), 0, s, b);
    hipLaunchKernelGGL(pjd_k_lane_dc_carry, dim3(1), dim3(256), 0, s, b);
}

// ... and for dense input
void pjd_launch_idct_dense(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const PjdDevIdctWg *wgs, const uint64_t *dense_base, uint32_t n_wg)
{
    if (n_wg == 0) return;
    static const PjdDenseKernel colour[2][2] = {{pjd_k_idct_colour_planar<true>, pjd_k_idct_colour_planar<false>},
                                                {pjd_k_idct_colour<true>, pjd_k_idct_colour<false>}};
    const PjdDenseKernel k = f.gray() ? pjd_gray_dense_kernel(f.scaled ? PJD_GRAY_SCALED : PJD_GRAY_FULL) : colour[f.layout != PJD_BACK_PLANAR][!f.scaled];
    hipLaunchKernelGGL(k, dim3(n_wg), dim3(PJD_IDCT_THREADS), 0, s, b, wgs, dense_base);
}
