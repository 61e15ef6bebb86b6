// pjd_k_blur_body.h -- the body of the blur kernels of pjd_k_blur.hip (pjd_batch_set_blur), included once per kernel as the resample
// bodies are: a textual include, so that tools/blur_host.cpp runs this very text on the host.
// One workgroup per tile of one output (the host's prefix sum over the outputs' tiles says which): PJD_BLUR_COLS x PJD_BLUR_ROWS samples,
// one channel at a time through three phases with a barrier between them --
//   stage:  the tile and its halo of r on every side as bytes in LDS, every index through the border rule (pjd_blur_index_calc), read from
//           U in the layout the resample wrote (plane by plane, or interleaved);
//   rows:   ONCE per staged row, four adjacent row samples per thread from a sliding window of the staged bytes (one byte read per tap),
//           h8 = tap_row(sum), 16 bits, into LDS;
//   cols:   a thread accumulates PJD_RS_PX adjacent columns of two adjacent rows in registers from a sliding window down the h8 rows (one
//           8-byte read per tap), and leaves the finished bytes in LDS --
// and, all channels done, out through the epilogue of the resample (store_row of pjd_k_resize_store.h, called as it is): a thread
// PJD_RS_PX adjacent pixels of a row, every element type and layout, vector stores where the address has their alignment.
// The arithmetic is the triangle filter's (tap_mac / tap_row / tap_out with PJD_RESIZE_ANTIALIAS; normative in include/pjd.h).  Everything
// up to the thread's own slot is uniform over the workgroup: the record, the tap count and the taps (read through an index that does not
// depend on the thread: scalar loads, the loop counts and weights in scalar registers, as in colour_px).  A record flagged
// PJD_BLUR_IDENTITY reads row 0 of the table, the one tap 65536: r = 0, no halo, and the same arithmetic is the copy.
// Only what the tile has is staged and computed: its rows rounded up to 2 and its columns to 4, which the border rule makes defined reads
// whatever the output's size; what lies beyond the output is never stored.  No thread leaves between the first barrier and the last.
// PJD_BLUR_T0 / _TSTEP say which items of a phase this thread takes (its own of the workgroup's here; all of them where a thread runs
// alone, on the host, where a barrier is nothing).
// In scope: PLANAR, DT, NC (compile-time constants; NC 3, or 1 only where PLANAR -- a grey batch), lds (dynamic LDS, 8-byte aligned),
// src, dst, recs, tile_prefix, taps, n_images, n_tiles, lds_bytes, nz (NormArgs; read only where DT != 0); tap_mac, tap_row, tap_out, store_row.
#ifndef PJD_BLUR_T0
#define PJD_BLUR_T0    threadIdx.x
#define PJD_BLUR_TSTEP PJD_BLUR_THREADS
#endif
    static_assert(PJD_BLUR_COLS == 16 * PJD_RS_PX && PJD_BLUR_ROWS * 8 == PJD_BLUR_THREADS && PJD_BLUR_THREADS == 256, "the slots below are written for 16 x 16 threads of 4 x 2 samples");
    static_assert(PJD_BLUR_COLS + PJD_BLUR_MAX_TAPS - 1 <= 128, "a staged row is at most 128 bytes: the staging loop takes 128 threads a row");
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles) return;                           // uniform, as everything up to the slots
    // the output of this tile: the last one whose prefix is <= tile (every output has a pixel, so a tile)
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    const PjdDevBlur b = recs[lo];
    const bool ident = (b.flags & PJD_BLUR_IDENTITY) != 0;
    const uint32_t ks = ident ? 1u : b.ksize, r = ks >> 1;
    const uint32_t *q = taps + (ident ? 0u : b.tap_off);
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t rowt = (t / b.col_tiles) * PJD_BLUR_ROWS, colt = (t % b.col_tiles) * PJD_BLUR_COLS;
    if (rowt >= b.th || colt >= b.tw || ks > PJD_BLUR_MAX_TAPS || pjd_blur_lds(r, NC) > lds_bytes) return;   // never with the host's records: nothing is read or written out of bounds
    const uint32_t n_rows = b.th - rowt < PJD_BLUR_ROWS ? b.th - rowt : PJD_BLUR_ROWS, n_cols = b.tw - colt < PJD_BLUR_COLS ? b.tw - colt : PJD_BLUR_COLS;
    const uint32_t gr = (n_rows + 1u) >> 1, gc = (n_cols + 3u) >> 2;       // the row pairs and column quads of the tile that hold a sample
    const uint32_t sr = 2u * gr + 2u * r, sc = 4u * gc + 2u * r;           // staged rows and columns
    const uint32_t pitch = pjd_blur_pitch(r);
    uint8_t *stage = reinterpret_cast<uint8_t *>(lds);                     // [PJD_BLUR_ROWS + 2r][pitch]
    uint16_t *h8 = reinterpret_cast<uint16_t *>(stage + (PJD_BLUR_ROWS + 2u * r) * pitch);   // [PJD_BLUR_ROWS + 2r][PJD_BLUR_COLS]
    uint8_t *fin = reinterpret_cast<uint8_t *>(h8 + (PJD_BLUR_ROWS + 2u * r) * PJD_BLUR_COLS);   // [NC][PJD_BLUR_ROWS][PJD_BLUR_COLS]
    const uint8_t *sp = src + b.src_off;
    const uint64_t plane = PLANAR ? (uint64_t)b.tw * b.th : 1u;

#pragma unroll 1
    for (int c = 0; c < NC; c++) {
        // stage: 128 threads a row
        for (uint32_t it = PJD_BLUR_T0; it < sr * 128u; it += PJD_BLUR_TSTEP) {
            const uint32_t sy = it >> 7, sx = it & 127u;
            if (sx < sc) {
                const uint32_t y = pjd_blur_index_calc(b.th, (int32_t)(rowt + sy) - (int32_t)r);
                const uint32_t x = pjd_blur_index_calc(b.tw, (int32_t)(colt + sx) - (int32_t)r);
                const uint64_t at = (uint64_t)y * b.tw + x;                // always inside the output
                stage[sy * pitch + sx] = PLANAR ? sp[(uint64_t)c * plane + at] : sp[3u * at + (uint32_t)c];
            }
        }
        __syncthreads();
        // rows: 16 threads a staged row, four row samples each
        for (uint32_t it = PJD_BLUR_T0; it < sr * 16u; it += PJD_BLUR_TSTEP) {
            const uint32_t sy = it >> 4, g = it & 15u;
            if (g < gc) {
                const uint8_t *p = stage + sy * pitch + 4u * g;
                uint32_t v0 = p[0], v1 = p[1], v2 = p[2], h0 = 0u, h1 = 0u, h2 = 0u, h3 = 0u;
                for (uint32_t j = 0; j < ks; j++) {
                    const uint32_t w = q[j], v3 = p[j + 3u];   // the last one read is byte 4g + 2r + 3 < sc
                    h0 = tap_mac<PJD_RESIZE_ANTIALIAS>(h0, w, v0);
                    h1 = tap_mac<PJD_RESIZE_ANTIALIAS>(h1, w, v1);
                    h2 = tap_mac<PJD_RESIZE_ANTIALIAS>(h2, w, v2);
                    h3 = tap_mac<PJD_RESIZE_ANTIALIAS>(h3, w, v3);
                    v0 = v1; v1 = v2; v2 = v3;
                }
                uint32_t *o = reinterpret_cast<uint32_t *>(h8 + sy * PJD_BLUR_COLS + 4u * g);
                o[0] = tap_row<PJD_RESIZE_ANTIALIAS>(h0) | (tap_row<PJD_RESIZE_ANTIALIAS>(h1) << 16);
                o[1] = tap_row<PJD_RESIZE_ANTIALIAS>(h2) | (tap_row<PJD_RESIZE_ANTIALIAS>(h3) << 16);
            }
        }
        __syncthreads();
        // cols: the thread's slot, four columns of rows 2 ly and 2 ly + 1 of the tile
        for (uint32_t slot = PJD_BLUR_T0; slot < PJD_BLUR_THREADS; slot += PJD_BLUR_TSTEP) {
            const uint32_t lx = slot & 15u, ly = slot >> 4;
            if (lx < gc && ly < gr) {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(h8 + 2u * ly * PJD_BLUR_COLS + 4u * lx);
                uint32_t a0[PJD_RS_PX] = {0u, 0u, 0u, 0u}, a1[PJD_RS_PX] = {0u, 0u, 0u, 0u};
                uint32_t c0 = p[0], c1 = p[1];
                for (uint32_t j = 0; j < ks; j++) {
                    const uint32_t w = q[j];
                    p += PJD_BLUR_COLS / 2;                    // the last row read is 2 ly + 2r + 1 < sr
                    const uint32_t n0 = p[0], n1 = p[1];
                    a0[0] = tap_mac<PJD_RESIZE_ANTIALIAS>(a0[0], w, c0 & 0xffffu); a0[1] = tap_mac<PJD_RESIZE_ANTIALIAS>(a0[1], w, c0 >> 16);
                    a0[2] = tap_mac<PJD_RESIZE_ANTIALIAS>(a0[2], w, c1 & 0xffffu); a0[3] = tap_mac<PJD_RESIZE_ANTIALIAS>(a0[3], w, c1 >> 16);
                    a1[0] = tap_mac<PJD_RESIZE_ANTIALIAS>(a1[0], w, n0 & 0xffffu); a1[1] = tap_mac<PJD_RESIZE_ANTIALIAS>(a1[1], w, n0 >> 16);
                    a1[2] = tap_mac<PJD_RESIZE_ANTIALIAS>(a1[2], w, n1 & 0xffffu); a1[3] = tap_mac<PJD_RESIZE_ANTIALIAS>(a1[3], w, n1 >> 16);
                    c0 = n0; c1 = n1;
                }
                uint32_t *o = reinterpret_cast<uint32_t *>(fin + ((uint32_t)c * PJD_BLUR_ROWS + 2u * ly) * PJD_BLUR_COLS + 4u * lx);
                o[0] = tap_out<PJD_RESIZE_ANTIALIAS>(a0[0]) | (tap_out<PJD_RESIZE_ANTIALIAS>(a0[1]) << 8) | (tap_out<PJD_RESIZE_ANTIALIAS>(a0[2]) << 16) | (tap_out<PJD_RESIZE_ANTIALIAS>(a0[3]) << 24);
                o[PJD_BLUR_COLS / 4] = tap_out<PJD_RESIZE_ANTIALIAS>(a1[0]) | (tap_out<PJD_RESIZE_ANTIALIAS>(a1[1]) << 8) | (tap_out<PJD_RESIZE_ANTIALIAS>(a1[2]) << 16) | (tap_out<PJD_RESIZE_ANTIALIAS>(a1[3]) << 24);
            }
        }
        // the next channel's staging writes bytes nobody reads any more; its rows phase starts behind a barrier that every thread passes
        // only with its columns done
    }
    __syncthreads();

    uint8_t *dp = dst + b.dst_off;
    const uint64_t dst_plane = PLANAR ? (uint64_t)b.tw * b.th : 1u;
    const uint32_t dst_stride = PLANAR ? b.tw : 3u * b.tw;
    for (uint32_t slot = PJD_BLUR_T0; slot < PJD_BLUR_THREADS; slot += PJD_BLUR_TSTEP) {
        const uint32_t lx = slot & 15u, ly = slot >> 4;
        const uint32_t col0 = colt + 4u * lx;
        if (lx < gc && col0 < b.tw) {
            const uint32_t n_px = b.tw - col0 < PJD_RS_PX ? b.tw - col0 : PJD_RS_PX;
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t row = rowt + 2u * ly + k;
                if (ly < gr && row < b.th) {
                    uint32_t px[3][PJD_RS_PX];
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const uint32_t d = *reinterpret_cast<const uint32_t *>(fin + ((uint32_t)c * PJD_BLUR_ROWS + 2u * ly + k) * PJD_BLUR_COLS + 4u * lx);
#pragma unroll
                        for (int e = 0; e < PJD_RS_PX; e++) px[c][e] = (d >> (8 * e)) & 255u;
                    }
                    store_row<PLANAR, DT, NC>(px, dp, row, col0, n_px, dst_plane, dst_stride, nz);
                }
            }
        }
    }
