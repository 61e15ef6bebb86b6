// pjd_k_idct_dense_body.h -- the body of the dense back-end kernels, included once per kernel by pjd_k_backend.hip:
// pjd_k_idct_colour<SCALED> with PJD_DENSE_PLANAR = false, pjd_k_idct_colour_planar<SCALED> with PJD_DENSE_PLANAR = true.
// One text for both, and textual inclusion rather than a shared function on purpose: with the body moved into a function,
// pjd_k_idct_colour<false> took three more registers (39 -> 42); included, it compiles to the instructions it had when it stood in
// the kernel (profiles/planar_output.md).  Uses the kernel's parameters B, wgs, dense_base and its template parameter SCALED.
#ifndef PJD_DENSE_PLANAR
#error "define PJD_DENSE_PLANAR (false / true) before including pjd_k_idct_dense_body.h"
#endif
    __shared__ __attribute__((aligned(16))) int16_t tile[PJD_IDCT_MAX_DU][TILE_STRIDE];
    __shared__ uint16_t qs[3][64];
    __shared__ uint32_t mcu_xy[PJD_IDCT_MAX_DU];

    const PjdDevIdctWg wg = wgs[blockIdx.x];
    const PjdDevImage &im = B.images[wg.image];
    const uint32_t tid = threadIdx.x;
    const uint32_t dus = im.dus_per_mcu, nl = im.n_luma;
    const uint32_t n_du = wg.n_mcu * dus;
    const uint32_t RI = im.restart_interval;

    if (tid < 192) qs[tid >> 6][tid & 63] = B.qtab[(size_t)wg.image * 192 + tid];
    __syncthreads();

    // ---- load (16 B per lane, coalesced), DC fix-up, de-zigzag, dequantise, row pass ----------
    // lane (du, r) owns zigzag slots 8r..8r+7 on load; after the scatter to natural order a
    // second sweep does the row pass.
    const int16_t *cbase = B.coef + (dense_base[wg.pad_] + (uint64_t)(wg.first_mcu - im.first_mcu) * dus) * 64;
    for (uint32_t i = tid; i < n_du * 8; i += PJD_IDCT_THREADS) {
        const uint32_t du = i >> 3, r = i & 7;
        const uint32_t ml = du / dus, k = du - ml * dus;
        const uint32_t comp = k < nl ? 0 : k - nl + 1;
        const int4 raw = *reinterpret_cast<const int4 *>(cbase + (size_t)du * 64 + r * 8);
        const int16_t *rv = reinterpret_cast<const int16_t *>(&raw);
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = rv[j];
        int16_t *t = tile[du];
        const uint16_t *q = qs[comp];
        // the sentinel means "explicit zero" at slot 52 of a baseline picture only; everywhere else -32768 is a value (an
        // absolute DC the int16 predictor reached, a progressive coefficient shifted by Al)
        const bool zero52 = r == 6 && !(im.flags & PJD_IF_PROGRESSIVE) && v[4] == PJD_COEF_SENTINEL;
        if (r == 6 && !(im.flags & PJD_IF_STANDARD_ZIGZAG)) {
            // slots 48..55.  Natural position 38 is the target of slot 48 AND slot 52 (the
            // reference's zigzag_map[48] = 38): the later write wins, and an explicit zero
            // written at slot 52 (run/size symbol with size 0) is marked by the sentinel.
            const int v52 = v[4];
            const int n38 = v52 != 0 ? (zero52 ? 0 : v52) : v[0];
            t[38] = (int16_t)pjd_dequant(n38, q[38]);
            t[59] = (int16_t)pjd_dequant(v[1], q[59]);
            t[52] = (int16_t)pjd_dequant(v[2], q[52]);
            t[45] = (int16_t)pjd_dequant(v[3], q[45]);
            t[31] = (int16_t)pjd_dequant(v[5], q[31]);
            t[39] = (int16_t)pjd_dequant(v[6], q[39]);
            t[46] = (int16_t)pjd_dequant(v[7], q[46]);
            t[58] = 0;                    // natural 58 is never written by the reference
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t nat = (r == 6 && j == 0) ? 58u : c_zz[r * 8 + j];          // r == 6 here: PJD_IF_STANDARD_ZIGZAG
                t[nat] = (int16_t)pjd_dequant(j == 4 && zero52 ? 0 : v[j], q[nat]);
            }
        }
    }
    __syncthreads();
    pjd_tile_to_pixels<true, SCALED, PJD_DENSE_PLANAR>(tile, mcu_xy, B, im, wg, tid);
