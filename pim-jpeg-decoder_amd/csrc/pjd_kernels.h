// pjd_kernels.h -- launchers of the gfx950 kernels (implemented in pjd_k_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pjd_internal.h"

// All device pointers of one batch, as the kernels see them.
struct PjdDevBatch {
    const PjdDevImage *images;
    const PjdDevTset *tsets;
    const PjdDevHuffRaw *raw_tables;     // n_tsets * PJD_MAX_TABLES
    uint8_t *luts;                       // decode tables, one blob per table set (PjdDevTset::lut_off16)
    const uint16_t *qtab;                // n_images * 3 * 64
    const PjdDevSegment *segs;
    const PjdDevSub *lanes;
    const PjdDevHuffWave *hwaves;
    const PjdDevHuffWg *hwgs;
    const PjdDevIdctWg *iwgs;
    const PjdDevScan *pscans;            // scans of the progressive frames of the batch (PjdDevImage::pscan_base)
    const uint32_t *group_images;        // picture groups (pjd_internal.h): image indices, group after group
    const uint32_t *iwg_order;           // ... and back-end workgroup indices (into iwgs / marks), group after group
    const uint8_t *ecs;
    uint32_t *words;                     // transposed bitstream words: [wave][PJD_WORD_ROWS][64]
    int16_t *coef;                       // DENSE scratch (exact-kernel path): dense_du * 64 int16, zigzag-slot order
    uint16_t *ent;                       // lane streams: lane q of image `im` owns slots [im.ent_base + (q - im.lane_base) * im.lane_cap, + im.lane_cap)
    PjdDevLaneInfo *lane_info;           // per lane
    PjdDevLaneDc *lane_dc;               // per lane
    uint16_t *dc_blk;                    // per DC scan block: aggregate {Y, Cb, Cr, has_head}, then carry-in {Y, Cb, Cr, -}
    PjdDevMark *marks;                   // per IDCT workgroup of the parallel path
    uint8_t *out;
    int32_t *status;                     // per image
    PjdDevImState *imstate;              // per image: first entropy-coding error / earliest unresolved irregularity of this decode
    // Huffman kernel scratch (zeroed before every launch)
    uint64_t *wave_gen;                  // [PJD_GENS][n_hwave]: exit state of a wave's last lane | flag, one word per generation (pjd_internal.h)
    uint64_t *wave_desc;                 // per Huffman wave: look-back descriptor (status | poison | head | units)
    uint32_t *ticket;                    // workgroup index dispenser
    uint32_t *dbg;                       // PJD_DEBUG_STATS: per wave, 8 timestamps (10 ns units); else null
    unsigned long long *stats;           // [16] diagnostics: 0 re-sync rounds, 1 lane passes in them, 2 / 3 the same for the stitch
                                         //      stage, PJD_STAT_FLAG0.. waves that flagged their image, by reason, 12 / 13 cooperative walks and the lanes walked in them
    uint32_t n_images, n_tsets, n_lanes, n_hwave, n_hwg, n_iwg, n_dcblk;
    uint32_t sub_bytes;                  // Huffman subsequence size of this batch
    uint32_t word_rows;                  // PJD_WORD_ROWS(sub_bytes)
    uint32_t lane_cap;                   // largest PjdDevImage::lane_cap of the batch (diagnostics)
    uint32_t max_lut_bytes;              // largest PjdDevTset::lut_bytes in the batch (sizes the dynamic LDS of the Huffman kernel)
};

// ---- back end (pjd_k_backend.hip) ------------------------------------------------
void pjd_launch_dpu_payload(hipStream_t s, const uint32_t *metadata, int16_t *mcus, int n_dpus);
void pjd_launch_zero(hipStream_t s, void *p, size_t bytes);          // bytes: a multiple of 16
void pjd_launch_reset(hipStream_t s, const PjdDevBatch &b, const int32_t *status_init, uint64_t *opstate, size_t opstate_words, uint32_t dbg_words);   // per-decode state
// ---- the fused back end: coefficients -> pixels, one kernel family per form of the batch's output
// The form: where the channels of a pixel go, and whether the batch holds pictures with an output scale (PJD_IF_SCALE_MASK: the
// kernels that also serve them).  Built once from the plan (pjd_batch::back, pjd_api.hip); every launcher below picks its kernel by it.
// Layouts: PJD_OUT_RGB8 and _BMP; PJD_OUT_RGB8_PLANAR (the _planar kernels); PJD_OUT_GRAY8 (pjd_k_backend_gray.hip: the luma units alone)
enum PjdBackLayout : uint8_t { PJD_BACK_INTERLEAVED = 0, PJD_BACK_PLANAR = 1, PJD_BACK_GRAY = 2 };
struct PjdBackForm {
    PjdBackLayout layout;
    bool scaled;
    bool planes() const { return layout != PJD_BACK_INTERLEAVED; }     // what the resample reads and writes: planes (three, or one)
    bool gray() const { return layout == PJD_BACK_GRAY; }
};
// lane-stream input: workgroup k takes range order[k] of iwgs / marks (null: the identity -- the whole batch when n_wg = n_iwg)
void pjd_launch_idct_lanes(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const uint32_t *order, uint32_t n_wg);
// dense input (exact path): wgs[k].pad_ = index into dense_base[] (data unit 0 of that image's scratch)
void pjd_launch_idct_dense(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const PjdDevIdctWg *wgs, const uint64_t *dense_base, uint32_t n_wg);
// verdict (status words) and DC predictors of the whole batch: one launch, a workgroup per picture (pjd_k_group_dc), or -- a batch with
// a picture of very many lanes, PjdPlan::dc_per_picture -- three: per-image verdict, local scan, carry
void pjd_launch_lane_dc_scan(hipStream_t s, const PjdDevBatch &b, bool per_picture);
// one picture group (pjd_internal.h): verdict + DC predictors of its pictures in one launch (its back-end workgroups: pjd_launch_idct_lanes)
void pjd_launch_group_dc(hipStream_t s, const PjdDevBatch &b, const PjdDevGroup &g);
// ---- PJD_F_LIBJPEG pictures (islow IDCT), from the lane streams or the dense scratch as above.  Interleaved and planar batches
// (pjd_k_backend_std.hip): into component planes -- `planes` is the batch's plane buffer (PjdDevImage::plane_off256) -- then upsample +
// colour + store by pjd_launch_colour_std (cwgs[k] = {image, first 4-pixel item, -, -}).  A grey batch (pjd_k_backend_gray.hip): the
// luma units straight into the picture; `planes` is unused and there is no colour launch.
// Every list has two parts: n_wg ranges (colour: workgroups of items) of pictures at full size, then n_red of pictures with
// PJD_F_LIBJPEG_SCALE_*, which take the _red kernels -- libjpeg's reduced IDCTs into planes of the reduced geometry, a reduced picture.
void pjd_launch_idct_std_lanes(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const uint32_t *order, uint32_t n_wg, uint32_t n_red, uint8_t *planes);
void pjd_launch_idct_std_dense(hipStream_t s, const PjdDevBatch &b, PjdBackForm f, const PjdDevIdctWg *wgs, const uint64_t *dense_base, uint32_t n_wg, uint32_t n_red,
                               uint8_t *planes);
void pjd_launch_colour_std(hipStream_t s, const PjdDevBatch &b, const PjdDevIdctWg *cwgs, uint32_t n_wg, uint32_t n_red, uint8_t *planes);
// ---- resize on decode (pjd_k_resize.hip): every picture of the batch from `src` (interleaved RGB8, or planar) to its target size in `dst`
// (the same layout), one launch whatever the batch asked for; tile_prefix[i] = tiles of the pictures before i, tile_prefix[n_images] =
// n_tiles.  norm.dtype != 0: the samples leave as fp16 / bf16 / fp32 elements, v * scale[c] + bias[c] (pjd_batch_set_normalize); the
// records' dst_off stay byte offsets.  win: null, or win[i] is picture i's source window, defaults resolved
// (pjd_batch_set_resize_window).  filter: PJD_RESIZE_* (pjd_batch_set_resize_filter); for the two table-driven ones aa[i] says where picture
// i's weights lie in `tab` (pjd_internal.h; the tables of the windowed axes where win), and lds_bytes is the largest row segment a tile
// of the batch stages (mirrored tiles included); all three unused otherwise.
struct PjdResizeLaunch {
    const uint8_t *src;
    uint8_t *dst;
    const PjdDevResize *recs;
    const uint32_t *tile_prefix;
    uint32_t n_images, n_tiles;
    bool planar;
    PjdNormalize norm;
    const PjdDevResizeWin *win;
    bool oriented;                       // pjd_batch_set_orientation: win is set, and its flags hold PJD_RWI_* (the ORI kernels)
    int filter;
    const PjdDevResizeAA *aa;
    const uint32_t *tab;
    uint32_t lds_bytes;
    const PjdDevResizePad *pad;          // pjd_batch_set_resize_pad: null, or win is set too and pad[i] is picture i's canvas (the PAD kernels)
    uint32_t channels = 3;               // 3, or 1 for a grey batch (PJD_OUT_GRAY8): planar, one plane, win and pad always set (the pjd_k_resize_gray kernels)
    const PjdDevColour *colour = nullptr; // pjd_batch_set_colour: null, or colour[i] is output i's map; win and pad always set, three channels (the pjd_k_resize_col kernels)
};
void pjd_launch_resize(hipStream_t s, const PjdResizeLaunch &a);
// ... and the border of its padded pictures (pjd_k_resize_border): line_prefix[i] = canvas lines (rows interleaved, plane rows planar) of
// the padded pictures before i, line_prefix[n_images] = n_lines; elem_bytes 1 (uint8), 2 or 4; fill: the pattern of PjdPadFill
struct PjdBorderLaunch {
    uint8_t *dst;
    const PjdDevResize *recs;
    const PjdDevResizePad *pad;
    const uint32_t *line_prefix;
    uint32_t n_images, n_lines;
    bool planar;
    uint32_t elem_bytes;
    PjdPadFill fill;
    uint32_t channels = 3;               // 3, or 1 for a grey batch: planar with ONE plane, n_lines counts H lines a canvas and fill.d[0] alone is read
};
void pjd_launch_resize_border(hipStream_t s, const PjdBorderLaunch &a);
// ---- affine warp on decode (pjd_k_warp.hip; pjd_batch_set_resize_affine): every output from its picture in `src` under its own inverse
// map warp[i] (pjd_internal.h) into `dst`, one launch that writes every byte; recs and tile_prefix as above, but in tiles of
// PJD_WARP_COLS x PJD_WARP_ROWS; fill: R | G << 8 | B << 16 (a grey batch: the low byte), a sample like any other under norm
struct PjdWarpLaunch {
    const uint8_t *src;
    uint8_t *dst;
    const PjdDevResize *recs;
    const PjdDevWarp *warp;
    const uint32_t *tile_prefix;
    uint32_t n_images, n_tiles;
    bool planar;
    PjdNormalize norm;
    uint32_t fill;
    uint32_t channels = 3;
    const PjdDevColour *colour = nullptr; // pjd_batch_set_colour: null, or colour[i] is output i's map, applied to the blend (the fill included); three channels (pjd_k_warp_col)
};
void pjd_launch_warp(hipStream_t s, const PjdWarpLaunch &a);
// ---- Gaussian blur on decode (pjd_k_blur.hip; pjd_batch_set_blur): every output from U in `src` (the blur intermediate: uint8, the
// batch's layout) through its own taps into `dst`, one launch that writes every byte; tile_prefix in tiles of PJD_BLUR_COLS x
// PJD_BLUR_ROWS; taps: the table recs[i].tap_off points into; lds_bytes: pjd_blur_lds of the batch's largest radius
struct PjdBlurLaunch {
    const uint8_t *src;
    uint8_t *dst;
    const PjdDevBlur *recs;
    const uint32_t *tile_prefix;
    const uint32_t *taps;
    uint32_t n_images, n_tiles;
    bool planar;
    PjdNormalize norm;
    uint32_t channels = 3;               // 3, or 1 for a grey batch: planar, one plane
    uint32_t lds_bytes = 0;
};
void pjd_launch_blur(hipStream_t s, const PjdBlurLaunch &a);
// ---- stage-level parity (pjd_k_coefdump.hip): coefficients in the reference's MCU_buffer layout; `out` is zeroed by the caller
void pjd_launch_coefdump_lanes(hipStream_t s, const PjdDevBatch &b, uint32_t image, uint32_t n_iwg, int16_t *out);
void pjd_launch_coefdump_dense(hipStream_t s, const PjdDevBatch &b, uint32_t image, const int16_t *scratch, uint32_t first_du, uint32_t n_du, int16_t *out);
// ---- entropy decode (pjd_k_huffman.hip, pjd_k_huffman_seq.hip) ---------------------
// exact kernel: image_list[k] decodes into the dense scratch from data unit dense_base[k]
void pjd_launch_huff_sequential(hipStream_t s, const PjdDevBatch &b, const uint32_t *image_list, const uint64_t *dense_base, uint32_t n);
void pjd_launch_huff_exact_lut(hipStream_t s, const PjdDevBatch &b, const uint32_t *image_list, const uint64_t *dense_base, uint32_t n);   // the exact decoder, table-driven
// progressive frames among image_list (the others are skipped): scan by scan into the dense scratch (pjd_k_progressive.hip)
void pjd_launch_progressive(hipStream_t s, const PjdDevBatch &b, const uint32_t *image_list, const uint64_t *dense_base, uint32_t n);
// once per upload (pjd_batch_upload), not per decode: no kernel of a decode writes luts or words
void pjd_launch_build_tables(hipStream_t s, const PjdDevBatch &b);
void pjd_launch_lane_words(hipStream_t s, const PjdDevBatch &b);     // bitstream -> per-lane big-endian words, transposed per wave
void pjd_launch_huff_lanes(hipStream_t s, const PjdDevBatch &b);     // synchronise + stitch + scan + write
// what the runtime says of that launch on the current device: workgroups of pjd_k_huff_lanes one CU holds at the batch's dynamic LDS
// (*lds_bytes: that size)
hipError_t pjd_huff_lanes_occupancy(const PjdDevBatch &b, int *workgroups_per_cu, size_t *lds_bytes);
void pjd_launch_huff_lanes_group(hipStream_t s, const PjdDevBatch &b, const PjdDevGroup &g, uint32_t group_index);   // the same for one picture group
