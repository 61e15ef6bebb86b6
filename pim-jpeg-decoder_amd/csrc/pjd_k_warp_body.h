// pjd_k_warp_body.h -- the body of the affine warp kernels of pjd_k_warp.hip (pjd_batch_set_resize_affine), included once per kernel as
// the resample bodies are: a textual include, so that tools/warp_host.cpp runs this very text on the host, thread by thread.
// One wave per tile of one output (the host's prefix sum over the outputs' tiles says which), a lane PJD_RS_PX adjacent pixels of each
// of its PJD_WARP_RPL rows, so that the epilogue of the resample (store_row, pjd_k_resize_store.h) applies as it is.
//   - The source position of a pixel is the fixed-point sum of include/pjd.h: the lane makes X and Y once, in 64 bits, for the first
//     pixel of its first row (pjd_warp_pos), steps them by 2 * LY * a01 / a11 from one of its rows to the next and by 2 * a00 / a10 from
//     pixel to pixel -- the same sum, term by term, and every partial sum below 2^62.3 (pjd_internal.h) -- and reads floor and weight
//     with pjd_warp_fix, the code pjd_warp_tap exports.  From there on everything is 32 bits.
//   - The four taps are guarded without a branch: the coordinates are clamped into the picture, the load is made, and the in-range
//     predicate selects the loaded sample or the fill.  No load leaves the source picture's bytes -- pictures lie back to back in the
//     intermediate buffer, a wrong address would read a neighbour silently.
//   - The blend and its one rounding are those of the bilinear resize.  A pixel wholly outside blends four fills: the fill itself.
// The tile is PJD_WARP_COLS x PJD_WARP_ROWS = 32 x 32: PJD_WARP_LX = 8 lanes along a row and eight down, four rows a lane, so that one load
// instruction of the wave reads the taps of 32 x 8 target pixels -- about as many cache lines under a quarter turn as under none.
// Measured on the MI355X against 32 x 64, 64 x 32, 128 x 16 and the resize tile's 256 x 8 (the same text, -DPJD_WARP_LX / -DPJD_WARP_RPL):
// pure scaling 0.44 / 0.50 / 0.40 / 0.41 / 0.41 ms, a quarter turn 0.54 / 0.56 / 1.13 / 1.51 / 2.03 ms for the 1024-picture batch
// (profiles/affine_warp.md).  No LDS.
// In scope: PLANAR, DT, COL, NC (compile-time constants; NC 3, or 1 only where PLANAR -- a grey batch; COL: colour is read, NC is 3), src, dst, recs, warp, colour, tile_prefix,
// n_images, n_tiles, fill (R | G << 8 | B << 16; grey: the low byte), nz (NormArgs; read only where DT != 0); colour_px, store_row.
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * PJD_WARP_WAVES + (threadIdx.x >> 6));
    if (tile >= n_tiles) return;
    // the output of this tile: the last one whose prefix is <= tile (every output has a pixel, so a tile)
    uint32_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    const PjdDevResize r = recs[lo];
    const PjdDevWarp m = warp[lo];
    PjdDevColour cm{};                                     // COL (pjd_batch_set_colour): the map of this OUTPUT, wave-uniform as r and m are
    if constexpr (COL) cm = colour[lo];
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_WARP_ROWS + lane / PJD_WARP_LX;       // the lane's first row
    const uint32_t col0 = (t % r.col_tiles) * PJD_WARP_COLS + (lane % PJD_WARP_LX) * PJD_RS_PX;
    if (col0 >= r.tw) return;
    const uint32_t n_px = r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX;
    const uint8_t *sp = src + r.src_off;
    uint8_t *dp = dst + r.dst_off;
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;
    const uint64_t dst_plane = PLANAR ? (uint64_t)r.tw * r.th : 1u;
    const uint32_t dst_stride = PLANAR ? r.tw : 3u * r.tw;
    const uint32_t fl[3] = {fill & 255u, (fill >> 8) & 255u, (fill >> 16) & 255u};

    int64_t Xr = pjd_warp_pos(m.a00, m.a01, m.b0, col0, row0), Yr = pjd_warp_pos(m.a10, m.a11, m.b1, col0, row0);
#pragma unroll
    for (int k = 0; k < PJD_WARP_RPL; k++) {
        const uint32_t row = row0 + (uint32_t)k * PJD_WARP_LY;
        if (row < r.th) {                                  // per lane where the tile has lanes down
            int64_t X = Xr, Y = Yr;
            uint32_t px[3][PJD_RS_PX];
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                int32_t x0, y0;
                uint32_t wx, wy;
                pjd_warp_fix(X, x0, wx);
                pjd_warp_fix(Y, y0, wy);
                X += 2 * m.a00; Y += 2 * m.a10;
                const int32_t x1 = x0 + 1, y1 = y0 + 1;
                const bool inx0 = (uint32_t)x0 < r.sw, inx1 = (uint32_t)x1 < r.sw, iny0 = (uint32_t)y0 < r.sh, iny1 = (uint32_t)y1 < r.sh;
                const int32_t xm = (int32_t)r.sw - 1, ym = (int32_t)r.sh - 1;
                const uint32_t cx0 = (uint32_t)(x0 < 0 ? 0 : x0 > xm ? xm : x0) * (PLANAR ? 1u : 3u), cx1 = (uint32_t)(x1 < 0 ? 0 : x1 > xm ? xm : x1) * (PLANAR ? 1u : 3u);
                const uint32_t cy0 = (uint32_t)(y0 < 0 ? 0 : y0 > ym ? ym : y0), cy1 = (uint32_t)(y1 < 0 ? 0 : y1 > ym ? ym : y1);
                const uint8_t *s0 = sp + (uint64_t)cy0 * r.src_stride, *s1 = sp + (uint64_t)cy1 * r.src_stride;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const uint8_t *c0 = s0 + c * src_plane, *c1 = s1 + c * src_plane;
                    const uint32_t v00 = c0[cx0], v01 = c0[cx1], v10 = c1[cx0], v11 = c1[cx1];     // always inside the picture
                    const uint32_t s00 = inx0 && iny0 ? v00 : fl[c], s01 = inx1 && iny0 ? v01 : fl[c];
                    const uint32_t s10 = inx0 && iny1 ? v10 : fl[c], s11 = inx1 && iny1 ? v11 : fl[c];
                    const uint32_t top = __umul24(256u - wx, s00) + __umul24(wx, s01), bot = __umul24(256u - wx, s10) + __umul24(wx, s11);
                    px[c][q] = (__umul24(256u - wy, top) + __umul24(wy, bot) + 32768u) >> 16;
                }
            }
            if constexpr (COL) colour_px(px, cm);          // the fill took part in the blend as any sample: it passes through the map
            store_row<PLANAR, DT, NC>(px, dp, row, col0, n_px, dst_plane, dst_stride, nz);
        }
        Xr += 2 * PJD_WARP_LY * m.a01; Yr += 2 * PJD_WARP_LY * m.a11;
    }
