// pjd_k_resize_aa_body.h -- the body of the table-driven (separable) resample kernels of pjd_k_resize.hip, included once per kernel:
// pjd_k_resize_aa<PLANAR, DT> and, with WIN, pjd_k_resize_win_aa<PLANAR, DT> (pjd_batch_set_resize_window) for the widened triangle
// filter, pjd_k_resize_cubic / pjd_k_resize_win_cubic for the bicubic one.  A wave STREAMS down the source rows its tile reads
// (pjd_k_resize.hip says how).  FILT (PJD_RESIZE_ANTIALIAS or PJD_RESIZE_BICUBIC, a compile-time constant) chooses the ARITHMETIC of a
// tap, of the row sample between the passes and of the final rounding (tap_mac, tap_row, tap_out of pjd_k_resize_store.h: unsigned
// with 8 fraction bits, or signed with 6 and one clamp); the streaming, the staging, the tables' layout and the guards are one text.  The taps are those of a source WINDOW (include/pjd.h), which without WIN
// is the identity window (pjd_resize_win_identity) and folds away:
//   - the tables are those of the axes (w.w, w.vw) and (w.h, w.vh); a column's entries are at index w.ox + i', i' the lane's column or
//     its mirror image (PJD_RW_HFLIP), a row's at w.oy + row; the tap-major rows are w.vw and w.vh long;
//   - `first` grows with the tap index, so a mirrored tile has its lowest taps at its LAST column: the staged segment runs from the
//     first tap of the lower end to the last tap of the higher one (pjd_resize_win_ends, which also sizes the LDS on the host);
//   - the segment starts at column w.x + xs of row w.y + y: any dword remainder occurs, whatever the picture's own alignment (the
//     dword that holds its first byte is the first one loaded, and the taps read behind the remainder `sh`);
//   - the guards are the window's: a table that would reach past w.w makes the tile return, rows end at w.h.
// No lane leaves before the last barrier; lanes right of the picture compute its last column and store nothing.
// A textual include, so that tools/resize_host.cpp runs this very text on the host; PJD_WIN_STAGE_FIRST / _STEP say which dwords of a
// segment this thread stages (its own of the wave's 64 here; all of them where a thread runs alone).
// In scope: PLANAR, DT, WIN, ORI (implies WIN), PAD (implies ORI), COL (colour is read; NC is 3), FILT, NC (compile-time constants; NC: the channels, 3, or 1 only where PLANAR: ONE plane segment in LDS), seg (LDS), src, dst, recs, win (read only where WIN),
// pad (read only where PAD), tile_prefix, n_images,
// n_tiles, aa, tab, lds_bytes, nz, colour (read only where COL, which implies ORI); colour_tile, store_row and store_cols.
#ifndef PJD_WIN_STAGE_FIRST
#define PJD_WIN_STAGE_FIRST lane
#define PJD_WIN_STAGE_STEP  64u
#endif
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles) return;                           // uniform, as everything up to `col0`
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    const PjdDevResize r = recs[lo];
    const PjdDevResizeWin w = WIN ? win[lo] : pjd_resize_win_identity(r);
    const PjdDevResizeAA a = aa[lo];
    PjdDevColour cm{};                                     // COL (pjd_batch_set_colour): the map of this OUTPUT, as in pjd_k_resize_body.h
    if constexpr (COL) cm = colour[lo];
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_RS_ROWS;
    const uint32_t colt = (t % r.col_tiles) * PJD_RS_COLS;
    const uint32_t col0 = colt + lane * PJD_RS_PX;
    const uint32_t *xt = tab + a.x_tab, *yt = tab + a.y_tab;
    const bool flip = (w.flags & PJD_RW_HFLIP) != 0;

    // the source columns of the tile, relative to the window
    const uint32_t col_last = colt + PJD_RS_COLS - 1u < r.tw ? colt + PJD_RS_COLS - 1u : r.tw - 1u;
    uint32_t end_lo, end_hi;
    pjd_resize_win_ends(w, r.tw, colt, col_last, end_lo, end_hi);
    const uint32_t head0 = xt[end_lo], head1 = xt[end_hi];
    const uint32_t xs = head0 & 0xffffu, xe = (head1 & 0xffffu) + (head1 >> 16), span = xe - xs;
    const uint32_t pitch = (span + 6u) & ~3u;              // bytes per plane segment (PLANAR)
    if (xe > w.w || xe <= xs || pjd_resize_aa_lds(span, PLANAR, NC) > lds_bytes) return;   // never with the host's table: nothing is read or written out of bounds

    // the source rows of the tile (relative to the window), and per target row its first tap and tap count
    uint32_t yf[PJD_RS_ROWS], yc[PJD_RS_ROWS];
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        const uint32_t row = row0 + k < r.th ? row0 + k : r.th - 1u;
        const uint32_t head = yt[w.oy + row];
        yf[k] = head & 0xffffu;
        yc[k] = row0 + k < r.th ? head >> 16 : 0u;         // rows below the picture take nothing
    }
    const uint32_t row_last = row0 + PJD_RS_ROWS - 1u < r.th ? row0 + PJD_RS_ROWS - 1u : r.th - 1u;
    const uint32_t head_l = yt[w.oy + row_last];
    const uint32_t ys = yf[0], ye_ = (head_l & 0xffffu) + (head_l >> 16), ye = ye_ < w.h ? ye_ : w.h;

    // per lane: the table index of its four columns (the picture's last one for those right of it) and their first taps in the segment
    uint32_t xi[PJD_RS_PX], xf[PJD_RS_PX];
#pragma unroll
    for (int q = 0; q < PJD_RS_PX; q++) {
        const uint32_t c = col0 + q < r.tw ? col0 + q : r.tw - 1u;
        xi[q] = w.ox + (flip ? r.tw - 1u - c : c);
        xf[q] = (xt[xi[q]] & 0xffffu) - xs;
    }
    const uint32_t n_px = col0 >= r.tw ? 0u : (r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX);
    const uint8_t *sp = src + r.src_off + (uint64_t)w.y * r.src_stride + (PLANAR ? w.x + xs : 3u * (w.x + xs));   // the segment in row 0 of the window
    // With PAD (pjd_batch_set_resize_pad): the canvas's row length, plane and origin for the stores, as in pjd_k_resize_body.h
    const PjdDevResizePad cv = PAD ? pad[lo] : PjdDevResizePad{};
    uint8_t *dp = dst + r.dst_off + (PAD ? ((uint64_t)cv.top * cv.W + cv.left) * (PLANAR ? 1u : 3u) * (DT == 0 ? 1u : PJD_DT_SIZE(DT)) : 0u);
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;        // the whole picture's plane
    const uint64_t dst_plane = PLANAR ? (PAD ? (uint64_t)cv.W * cv.H : (uint64_t)r.tw * r.th) : 1u;
    const uint32_t dst_stride = PAD ? (PLANAR ? cv.W : 3u * cv.W) : (PLANAR ? r.tw : 3u * r.tw);
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(seg);

    uint32_t acc[PJD_RS_ROWS][3][PJD_RS_PX];
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++)
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] = 0u;

    for (uint32_t y = ys; y < ye; y++) {
        __syncthreads();                                   // the taps of the row before have been read
        uint32_t sh[3];                                    // bytes between the first dword staged and the segment's first byte
        if (PLANAR) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const uint8_t *g = sp + c * src_plane + (uint64_t)y * r.src_stride;
                sh[c] = (uint32_t)((uintptr_t)g & 3u);
                const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g - sh[c]);
                const uint32_t nd = (sh[c] + span + 3u) >> 2;
                for (uint32_t d = PJD_WIN_STAGE_FIRST; d < nd; d += PJD_WIN_STAGE_STEP) seg[c * (pitch >> 2) + d] = g4[d];
            }
        } else {
            const uint8_t *g = sp + (uint64_t)y * r.src_stride;
            sh[0] = (uint32_t)((uintptr_t)g & 3u);
            const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g - sh[0]);
            const uint32_t nd = (sh[0] + 3u * span + 3u) >> 2;
            for (uint32_t d = PJD_WIN_STAGE_FIRST; d < nd; d += PJD_WIN_STAGE_STEP) seg[d] = g4[d];
        }
        __syncthreads();

        uint32_t h[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) h[c][q] = 0u;
        for (uint32_t tp = 0; tp < a.x_taps; tp++) {
            const uint32_t *wrow = xt + (size_t)(tp + 1u) * w.vw;
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                const uint32_t wt = wrow[xi[q]];
                const uint32_t j = xf[q] + tp < span ? xf[q] + tp : span - 1u;    // past the column's count the weight is 0: any staged byte
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const uint32_t v = PLANAR ? sb[c * pitch + sh[c] + j] : sb[sh[0] + 3u * j + c];
                    h[c][q] = tap_mac<FILT>(h[c][q], wt, v);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) h[c][q] = tap_row<FILT>(h[c][q]);

#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) {
            const uint32_t d = y - yf[k];                  // wraps where the row's taps start below y
            if (d < yc[k]) {                               // uniform
                const uint32_t wt = yt[(size_t)(d + 1u) * w.vh + w.oy + row0 + k];
#pragma unroll
                for (int c = 0; c < NC; c++)
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] = tap_mac<FILT>(acc[k][c][q], wt, h[c][q]);
            }
        }
    }

    // With COL (pjd_batch_set_colour) the whole tile is finished in place first and goes through the output's map under one branch
    // (colour_tile); rows below the picture hold zeros, are mapped with the rest and never stored.  Then the two epilogues, as below:
    // the store_cols call and the store_row loop here are COPIES of the ones behind this block, less their tap_out, and must stay in
    // step with them -- an argument changed there is changed here.  The text behind this block was left word for word as it was, so
    // that the uncoloured kernels keep their instructions (tools/kernel_text.py compares them with the commit before); sharing one
    // store loop between the two has not been tried against that comparison.
    if constexpr (COL) {
#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++)
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] = tap_out<FILT>(acc[k][c][q]);
        colour_tile(acc, cm);
        if (w.flags & PJD_RWI_TRANSPOSE) {                 // uniform
            store_cols<PLANAR, DT, NC>(acc, dp, row0, r.th - row0 < PJD_RS_ROWS ? r.th - row0 : PJD_RS_ROWS, col0, n_px, (w.flags & PJD_RWI_YMIRROR) != 0, r.th, PAD ? cv.W : r.th, dst_plane, nz);
            return;
        }
#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) {
            if (row0 + k >= r.th) break;                   // uniform
            uint32_t px[3][PJD_RS_PX];
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int q = 0; q < PJD_RS_PX; q++) px[c][q] = acc[k][c][q];
            store_row<PLANAR, DT, NC>(px, dp, (w.flags & PJD_RWI_YMIRROR) ? r.th - 1u - (row0 + k) : row0 + k, col0, n_px, dst_plane, dst_stride, nz);
        }
        return;
    }
    // With ORI (pjd_batch_set_orientation) the picture's flags say where the rows go: a transposed picture's leave as columns
    // (store_cols), another one's at their own place or its mirror image.  The mirror is in the STORE row: the span ys..ye above
    // assumes that the tile's taps ascend with its rows.
    if constexpr (ORI) {
        if (w.flags & PJD_RWI_TRANSPOSE) {                 // uniform
#pragma unroll
            for (int k = 0; k < PJD_RS_ROWS; k++)
#pragma unroll
                for (int c = 0; c < NC; c++)
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++) acc[k][c][q] = tap_out<FILT>(acc[k][c][q]);
            store_cols<PLANAR, DT, NC>(acc, dp, row0, r.th - row0 < PJD_RS_ROWS ? r.th - row0 : PJD_RS_ROWS, col0, n_px, (w.flags & PJD_RWI_YMIRROR) != 0, r.th, PAD ? cv.W : r.th, dst_plane, nz);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        if (row0 + k >= r.th) break;                       // uniform
        uint32_t px[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) px[c][q] = tap_out<FILT>(acc[k][c][q]);
        store_row<PLANAR, DT, NC>(px, dp, ORI && (w.flags & PJD_RWI_YMIRROR) ? r.th - 1u - (row0 + k) : row0 + k, col0, n_px, dst_plane, dst_stride, nz);
    }
