// pjd_k_resize_store_body.h -- the epilogue of every resample kernel, ONE text: one target row of a lane, px[c][q] (q < n_px; 0: nothing),
// rounded to 8 bits, leaves as uint8 or as normalised fp16 / bf16 / fp32 elements for row `row`, columns col0.. of the picture at dp.  The
// widest store where the address has its alignment and all four pixels exist, element stores otherwise (pjd_batch_bind_output promises
// element alignment, no more).  The body of store_row (pjd_k_resize_store.h); pjd_k_resize_body.h says who includes it directly.
// In scope: PLANAR, DT, NC (compile-time constants; NC: the planes a PLANAR picture has, 3 or 1), px, dp, row, col0, n_px, dst_plane, dst_stride, nz (NormArgs; read only where DT != 0).
        if constexpr (DT != 0) {
            constexpr uint32_t ES = PJD_DT_SIZE(DT);       // bytes per element
            if (PLANAR) {
#pragma unroll
                for (int c = 0; c < NC; c++) {
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
            for (int c = 0; c < NC; c++) {
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
