// pjd_k_resize_body.h -- the body of the resample kernels of pjd_k_resize.hip, included once per kernel (as pjd_k_idct_dense_body.h is):
// pjd_k_resize<PLANAR> (uint8 pictures, DT = 0) and pjd_k_resize_norm<PLANAR, DT> (pjd_batch_set_normalize, DT = PJD_DT_*, elements of
// PJD_DT_SIZE(DT) bytes).  Taps and blends are this one text; the epilogue -- convert, pack, store -- is chosen by DT at compile time.
// A textual include and not a function both kernels call: the uint8 kernels then compile to the instructions they had before the
// float variants existed (profiles/normalized_output.md), which an inlined function did not give.
// In scope: PLANAR, DT (compile-time constants), src, dst, recs, tile_prefix, n_images, n_tiles, nz (NormArgs; read only where DT != 0;
// r.dst_off stays a byte offset).
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
    const uint32_t t = tile - tile_prefix[lo];
    const uint32_t row0 = (t / r.col_tiles) * PJD_RS_ROWS;
    const uint32_t col0 = (t % r.col_tiles) * PJD_RS_COLS + lane * PJD_RS_PX;

    // row taps: lane k (k < PJD_RS_ROWS) computes those of row row0 + k, and they are read back as scalars (y0 | wy << 16) here, while
    // every lane is still active
    uint32_t rowtap[PJD_RS_ROWS];
    {
        const uint32_t row = row0 + (lane & (PJD_RS_ROWS - 1));
        uint32_t y0, y1, wy;
        pjd_resize_tap_calc(r.sh, r.th, row < r.th ? row : r.th - 1, y0, y1, wy);
        const uint32_t packed = y0 | (wy << 16);
#pragma unroll
        for (int k = 0; k < PJD_RS_ROWS; k++) rowtap[k] = __builtin_amdgcn_readlane(packed, k);
    }
    if (col0 >= r.tw) return;                              // only now: the lanes that computed row taps may have no column

    uint32_t x0[PJD_RS_PX], x1[PJD_RS_PX], wx[PJD_RS_PX];
#pragma unroll
    for (int k = 0; k < PJD_RS_PX; k++) {
        const uint32_t x = col0 + k;
        pjd_resize_tap_calc(r.sw, r.tw, x < r.tw ? x : r.tw - 1, x0[k], x1[k], wx[k]);
        if (!PLANAR) { x0[k] *= 3u; x1[k] *= 3u; }          // byte offsets in an interleaved row
    }
    const uint32_t n_px = r.tw - col0 < PJD_RS_PX ? r.tw - col0 : PJD_RS_PX;
    const uint8_t *sp = src + r.src_off;
    uint8_t *dp = dst + r.dst_off;
    const uint64_t src_plane = PLANAR ? (uint64_t)r.src_stride * r.sh : 1u;        // from one channel to the next
    const uint64_t dst_plane = PLANAR ? (uint64_t)r.tw * r.th : 1u;
    const uint32_t dst_stride = PLANAR ? r.tw : 3u * r.tw;

#pragma unroll
    for (int k = 0; k < PJD_RS_ROWS; k++) {
        const uint32_t row = row0 + k;
        if (row >= r.th) break;                            // uniform
        const uint32_t y0 = rowtap[k] & 0xffffu, wy = rowtap[k] >> 16, y1 = y0 + 1u < r.sh ? y0 + 1u : r.sh - 1u;
        const uint8_t *s0 = sp + (uint64_t)y0 * r.src_stride, *s1 = sp + (uint64_t)y1 * r.src_stride;
        uint32_t px[3][PJD_RS_PX];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t *c0 = s0 + c * src_plane, *c1 = s1 + c * src_plane;
#pragma unroll
            for (int q = 0; q < PJD_RS_PX; q++) {
                const uint32_t top = lerp8(c0[x0[q]], c0[x1[q]], wx[q]), bot = lerp8(c1[x0[q]], c1[x1[q]], wx[q]);
                px[c][q] = (__umul24(256u - wy, top) + __umul24(wy, bot) + 32768u) >> 16;
            }
        }
        if constexpr (DT != 0) {
            constexpr uint32_t ES = PJD_DT_SIZE(DT);       // bytes per element
            if (PLANAR) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    uint8_t *o = dp + ((uint64_t)c * dst_plane + (uint64_t)row * dst_stride + col0) * ES;
                    if (DT == PJD_DT_F32) {
                        if (n_px == PJD_RS_PX && ((uintptr_t)o & 15u) == 0) {
                            const f32x4 v = {pjd_normalize_f32(px[c][0], nz.scale[c], nz.bias[c]), pjd_normalize_f32(px[c][1], nz.scale[c], nz.bias[c]),
                                             pjd_normalize_f32(px[c][2], nz.scale[c], nz.bias[c]), pjd_normalize_f32(px[c][3], nz.scale[c], nz.bias[c])};
                            *reinterpret_cast<f32x4 *>(o) = v;
                        } else {
                            for (uint32_t q = 0; q < n_px; q++) reinterpret_cast<float *>(o)[q] = pjd_normalize_f32(px[c][q], nz.scale[c], nz.bias[c]);
                        }
                    } else {
                        const uint32_t lo = norm_pair16<DT>(px[c][0], px[c][1], nz.scale[c], nz.bias[c]);
                        const uint32_t hi = norm_pair16<DT>(px[c][2], px[c][3], nz.scale[c], nz.bias[c]);
                        if (n_px == PJD_RS_PX && ((uintptr_t)o & 7u) == 0) {
                            *reinterpret_cast<u32x2 *>(o) = u32x2{lo, hi};
                        } else {
                            for (uint32_t q = 0; q < n_px; q++) reinterpret_cast<uint16_t *>(o)[q] = (uint16_t)((q & 2u ? hi : lo) >> (16u * (q & 1u)));
                        }
                    }
                }
            } else {
                uint8_t *o = dp + ((uint64_t)row * dst_stride + 3u * col0) * ES;
                if (DT == PJD_DT_F32) {
                    float e[3 * PJD_RS_PX];                // R0 G0 B0 R1 ...
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++)
#pragma unroll
                        for (int c = 0; c < 3; c++) e[3 * q + c] = pjd_normalize_f32(px[c][q], nz.scale[c], nz.bias[c]);
                    if (n_px == PJD_RS_PX && ((uintptr_t)o & 15u) == 0) {
                        f32x4 *o4 = reinterpret_cast<f32x4 *>(o);
                        o4[0] = f32x4{e[0], e[1], e[2], e[3]};
                        o4[1] = f32x4{e[4], e[5], e[6], e[7]};
                        o4[2] = f32x4{e[8], e[9], e[10], e[11]};
                    } else {
#pragma unroll
                        for (int q = 0; q < PJD_RS_PX; q++)
                            if ((uint32_t)q < n_px)
#pragma unroll
                                for (int c = 0; c < 3; c++) reinterpret_cast<float *>(o)[3 * q + c] = e[3 * q + c];
                    }
                } else {
                    // six dwords: R0G0 B0R1 G1B1 R2G2 B2R3 G3B3 -- a pair spans two channels, so the elements are made one by one
                    uint32_t h[3 * PJD_RS_PX];
#pragma unroll
                    for (int q = 0; q < PJD_RS_PX; q++)
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float u = pjd_normalize_f32(px[c][q], nz.scale[c], nz.bias[c]);
                            h[3 * q + c] = DT == PJD_DT_F16 ? (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)u) : (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)u);
                        }
                    if (n_px == PJD_RS_PX && ((uintptr_t)o & 7u) == 0) {
                        u32x2 *o2 = reinterpret_cast<u32x2 *>(o);
                        o2[0] = u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
                        o2[1] = u32x2{h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
                        o2[2] = u32x2{h[8] | (h[9] << 16), h[10] | (h[11] << 16)};
                    } else {
#pragma unroll
                        for (int q = 0; q < PJD_RS_PX; q++)
                            if ((uint32_t)q < n_px)
#pragma unroll
                                for (int c = 0; c < 3; c++) reinterpret_cast<uint16_t *>(o)[3 * q + c] = (uint16_t)h[3 * q + c];
                    }
                }
            }
        } else if (PLANAR) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                uint8_t *o = dp + c * dst_plane + (uint64_t)row * dst_stride + col0;
                if (n_px == PJD_RS_PX && ((uintptr_t)o & 3u) == 0)
                    *reinterpret_cast<uint32_t *>(o) = px[c][0] | (px[c][1] << 8) | (px[c][2] << 16) | (px[c][3] << 24);
                else
                    for (uint32_t q = 0; q < n_px; q++) o[q] = (uint8_t)px[c][q];
            }
        } else {
            uint8_t *o = dp + (uint64_t)row * dst_stride + 3u * col0;
            if (n_px == PJD_RS_PX && ((uintptr_t)o & 3u) == 0) {
                struct alignas(4) U3 { uint32_t a, b, c; } v;
                v.a = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[0][1] << 24);
                v.b = px[1][1] | (px[2][1] << 8) | (px[0][2] << 16) | (px[1][2] << 24);
                v.c = px[2][2] | (px[0][3] << 8) | (px[1][3] << 16) | (px[2][3] << 24);
                *reinterpret_cast<U3 *>(o) = v;
            } else {
                for (uint32_t q = 0; q < n_px; q++)
                    for (int c = 0; c < 3; c++) o[3 * q + c] = (uint8_t)px[c][q];
            }
        }
    }
