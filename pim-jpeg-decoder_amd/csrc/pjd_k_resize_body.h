// pjd_k_resize_body.h -- the body of the bilinear resample kernels of pjd_k_resize.hip, included once per kernel (as
// pjd_k_idct_dense_body.h is): pjd_k_resize<PLANAR> (uint8 pictures, DT = 0), pjd_k_resize_norm<PLANAR, DT> (pjd_batch_set_normalize,
// DT = PJD_DT_*) and, with WIN, pjd_k_resize_win<PLANAR, DT> (pjd_batch_set_resize_window).  One wave per tile, a lane PJD_RS_PX adjacent
// pixels of each of its rows.  The taps are those of a source WINDOW (include/pjd.h), which without WIN is the identity window
// (pjd_resize_win_identity) and folds away: those kernels compile to the instructions they had before windows existed.
//   - column taps are pjd_resize_tap_calc(w.w, w.vw, w.ox + i'), i' the lane's column or its mirror image (PJD_RW_HFLIP); the lane
//     keeps its four target columns and their store order, only the tap index is mirrored;
//   - row taps are pjd_resize_tap_calc(w.h, w.vh, w.oy + row), and y1 clamps to the window's last row, not the picture's;
//   - both address the source from (w.x, w.y) on; the plane stride of a planar source stays the whole picture's (r.sh).
// A textual include and not a function the kernels call: the uint8 kernels then compile to the instructions they had before the float
// variants existed (profiles/normalized_output.md), which an inlined function did not give; and tools/resize_host.cpp runs this very
// text on the host.
// With ORI (which implies WIN) the store side reads the orientation of pjd_batch_set_orientation from the window's flags (PJD_RWI_* of
// pjd_internal.h); the read side does not know of it: the tap mirror is the bit PJD_RW_HFLIP has.
// In scope: PLANAR, DT, WIN, ORI, PAD, COL, NC (compile-time constants; PAD implies ORI; COL: colour is read, NC is 3; NC: the channels, 3, or 1 only where PLANAR -- a grey batch), src, dst, recs, win (read only where WIN), pad (read only where PAD), colour (read only where COL), tile_prefix, n_images, n_tiles, nz
// (NormArgs; read only where DT != 0; r.dst_off stays a byte offset); lerp8, colour_px, store_row and store_cols.
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
    const PjdDevResizeWin w = WIN ? win[lo] : pjd_resize_win_identity(r);
    PjdDevColour cm{};                                     // COL (pjd_batch_set_colour): the map of this OUTPUT, wave-uniform as r and w are
    if constexpr (COL) cm = colour[lo];
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_RS_ROWS;
    const uint32_t col0 = (t % r.col_tiles) * PJD_RS_COLS + lane * PJD_RS_PX;

    // row taps: lane k (k < PJD_RS_ROWS) computes those of row row0 + k, and they are read back as scalars (y0 in the window | wy << 16)
    // here, while every lane is still active
    uint32_t rowtap[PJD_RS_ROWS];
    {
        const uint32_t row = row0 + (lane & (PJD_RS_ROWS - 1));
        uint32_t y0, y1, wy;
        pjd_resize_tap_calc(w.h, w.vh, w.oy + (row < r.th ? row : r.th - 1), y0, y1, wy);
        const uint32_t packed = y0 | (wy << 16);
#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) rowtap[k] = __builtin_amdgcn_readlane(packed, k);
    }
    if (col0 >= r.tw) return;                              // only now: the lanes that computed row taps may have no column

    const bool flip = (w.flags & PJD_RW_HFLIP) != 0;
    uint32_t x0[PJD_RS_PX], x1[PJD_RS_PX], wx[PJD_RS_PX];
#pragma unroll
    for (int k = 0; k < PJD_RS_PX; k++) {
        const uint32_t c = col0 + k < r.tw ? col0 + k : r.tw - 1;
        pjd_resize_tap_calc(w.w, w.vw, w.ox + (flip ? r.tw - 1u - c : c), x0[k], x1[k], wx[k]);
        x0[k] += w.x; x1[k] += w.x;                        // x1 was clamped to the window: nothing right of it is read
        if (!PLANAR) { x0[k] *= 3u; x1[k] *= 3u; }          // byte offsets in an interleaved row
    }
    const uint32_t n_px = r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX;
    const uint8_t *sp = src + r.src_off + (uint64_t)w.y * r.src_stride;           // row 0 of the window
    // With PAD (pjd_batch_set_resize_pad) the picture is a rectangle of a canvas: the row length, the plane and the origin of the stores
    // are the canvas's (PjdDevResizePad), everything else -- tiles, taps, mirror extents -- stays the content's
    const PjdDevResizePad cv = PAD ? pad[lo] : PjdDevResizePad{};
    uint8_t *dp = dst + r.dst_off + (PAD ? ((uint64_t)cv.top * cv.W + cv.left) * (PLANAR ? 1u : 3u) * (DT == 0 ? 1u : PJD_DT_SIZE(DT)) : 0u);
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;        // from one channel to the next: the whole picture's plane
    const uint64_t dst_plane = PLANAR ? (PAD ? (uint64_t)cv.W * cv.H : (uint64_t)r.tw * r.th) : 1u;
    const uint32_t dst_stride = PAD ? (PLANAR ? cv.W : 3u * cv.W) : (PLANAR ? r.tw : 3u * r.tw);

    uint32_t kept[PJD_RS_ROWS][3][PJD_RS_PX] = {};         // ORI, a transposed picture: the rows of the tile (rows below the picture: 0, never stored); unused otherwise
#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        const uint32_t row = row0 + k;
        if (row >= r.th) break;                            // uniform
        const uint32_t y0 = rowtap[k] & 0xffffu, wy = rowtap[k] >> 16, y1 = y0 + 1u < w.h ? y0 + 1u : w.h - 1u;
        const uint8_t *s0 = sp + (uint64_t)y0 * r.src_stride, *s1 = sp + (uint64_t)y1 * r.src_stride;
        uint32_t px[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const uint8_t *c0 = s0 + c * src_plane, *c1 = s1 + c * src_plane;
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                const uint32_t top = lerp8(c0[x0[q]], c0[x1[q]], wx[q]), bot = lerp8(c1[x0[q]], c1[x1[q]], wx[q]);
                px[c][q] = (__umul24(256u - wy, top) + __umul24(wy, bot) + 32768u) >> 16;
            }
        }
        if constexpr (COL) colour_px(px, cm);              // the finished row, all three channels in registers: before either epilogue
        // The epilogue is one text in two forms, and the form is the only thing the two sides do not share: the kernels without a window
        // include it here, the windowed ones (and the antialiased body) call it as store_row.  The split is for the compiler's sake
        // alone: at -O3 either swap changes the instructions of all eight kernels of the side swapped (profiles/resize_unified.md), and
        // the two forms have not been timed against each other on a device.  Whoever has those timings can drop it.
        // With ORI (pjd_batch_set_orientation) the picture's flags say where the row goes: to its own place or its mirror image, or --
        // transposed -- nowhere yet: the tile keeps its rows, and they leave as columns behind the loop (store_cols).
        if constexpr (ORI) {
            if (w.flags & PJD_RWI_TRANSPOSE) {             // uniform
#pragma unroll
                for (int c = 0; c < NC; c++)
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++) kept[k][c][q] = px[c][q];
            } else {
                store_row<PLANAR, DT, NC>(px, dp, (w.flags & PJD_RWI_YMIRROR) ? r.th - 1u - row : row, col0, n_px, dst_plane, dst_stride, nz);
            }
        } else if constexpr (WIN) {
            store_row<PLANAR, DT, NC>(px, dp, row, col0, n_px, dst_plane, dst_stride, nz);
        } else {
#include "pjd_k_resize_store_body.h"
        }
    }
    if constexpr (ORI) {
        if (w.flags & PJD_RWI_TRANSPOSE)
            store_cols<PLANAR, DT, NC>(kept, dp, row0, r.th - row0 < PJD_RS_ROWS ? r.th - row0 : PJD_RS_ROWS, col0, n_px, (w.flags & PJD_RWI_YMIRROR) != 0, r.th, PAD ? cv.W : r.th, dst_plane, nz);
    }
