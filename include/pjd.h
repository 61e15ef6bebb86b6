/*
 * pjd.h -- C ABI of the MI355X-native JPEG decode path (libpjd.so).
 *
 * This is the drop-in boundary for the UPMEM-DPU dispatch of
 * jeun-990806/pim-jpeg-decoder.  Every entry point names the reference
 * interface it replaces (paths relative to the reference tree).
 *
 *   reference                                         this library
 *   ------------------------------------------------  -------------------------------
 *   DpuSet::allocate + load   decoder_host.cpp:32,268   pjd_open / pjd_close
 *   decode_Huffman_data       jpeg_scanner.cpp:707      \
 *   copy("metadata_buffer")   decoder_host.cpp:276       |  pjd_batch_create + _upload
 *   copy("mcus")              decoder_host.cpp:277      /
 *   exec()                    decoder_host.cpp:292      pjd_batch_decode (+ _sync)
 *   copy(batch.mcus,"mcus")   decoder_host.cpp:308      pjd_batch_download
 *   4 x dpus()[0]->copy(ctr)  decoder_host.cpp:309-312  pjd_batch_decode_timed
 *   one picture over all DPUs decoder_host.cpp:125-149   pjd_split_decode (restart segments over GPUs)
 *   the per-DPU payload T0    decoder_dpu.c:57-58       pjd_exec_dpu_payload (literal)
 *   (none: an addition)                                 PJD_F_SCALE_* + pjd_image_output_size: pictures out at
 *                                                       1/2, 1/4 or 1/8 scale (libjpeg scale_num/scale_denom)
 *   (none: an addition)                                 PJD_OUT_RGB8_PLANAR + pjd_batch_bind_output: pictures as planar
 *                                                       R, G, B channels in device memory the caller owns (tensors)
 *   (none: an addition)                                 pjd_batch_set_resize + pjd_resize_tap: every picture of a ragged batch
 *                                                       resampled to a size of its own inside the decode (one [N,3,H,W] tensor)
 *   (none: an addition)                                 pjd_batch_set_resize_filter + pjd_resize_aa_taps: that resize with the
 *                                                       antialiased triangle filter (torch antialias=True, Pillow BILINEAR)
 *   (none: an addition)                                 pjd_batch_set_resize_window + pjd_resize_window_check: that resize from a
 *                                                       window of the picture (RandomResizedCrop, Resize + CenterCrop, flip)
 *   (none: an addition)                                 pjd_batch_set_orientation: the eight EXIF orientations (mirrors, half turn,
 *                                                       quarter turns) per picture inside that launch (pjd_scanned_orientation reads the tag)
 *   (none: an addition)                                 pjd_batch_set_resize_pad + _set_pad_value + pjd_resize_pad_check: the picture keeps
 *                                                       its aspect ratio inside a fixed canvas and the rest is filled in that launch
 *                                                       (letterbox: YOLO, DETR, SAM, "expand to square")
 *   (none: an addition)                                 pjd_batch_set_normalize + pjd_normalize_value: the samples leave as fp16, bf16
 *                                                       or fp32, v * scale[c] + bias[c], in that launch (the tensor a model takes)
 *   (none: an addition)                                 PJD_F_LIBJPEG + pjd_libjpeg_idct / _ycc_to_rgb / _upsample_row: the picture libjpeg
 *                                                       decodes, bit for bit (islow IDCT, fancy upsampling, JFIF colour), per picture
 *   (none: an addition)                                 PJD_OUT_GRAY8 + pjd_output_channels: pictures as ONE 8-bit plane, the luma as libjpeg's
 *                                                       JCS_GRAYSCALE delivers it (a third of the bytes, no chroma work in the back end)
 *   (none: an addition)                                 PJD_F_LIBJPEG_SCALE_* + pjd_libjpeg_idct_scaled: libjpeg's reduced decode at 1/2, 1/4,
 *                                                       1/8 (its scaled IDCTs: Pillow's draft(), OpenCV's IMREAD_REDUCED_*), bit for bit
 *   (none: an addition)                                 pjd_batch_set_views + pjd_batch_n_outputs: several resampled outputs of one decoded
 *                                                       picture (two augmented views, multi-crop, FiveCrop, two resolutions, tiles): the
 *                                                       entropy decoder and the back end run once per picture, the resample once per view
 *   (none: an addition)                                 pjd_batch_set_resize_affine + pjd_warp_tap + pjd_resize_affine_check: every output under
 *                                                       an inverse 2 x 3 map of its own -- rotation, scale, shear, translation, a fill outside --
 *                                                       in one launch (RandomRotation, RandomAffine, DALI warp_affine, RandAugment)
 *   (none: an addition)                                 pjd_batch_set_colour + pjd_colour_value + pjd_colour_check: every output's 8-bit triple
 *                                                       through a 3 x 4 colour map of its own inside that launch (ColorJitter,
 *                                                       RandomGrayscale, BGR, DALI color_twist / hsv / brightness_contrast)
 *   (none: an addition)                                 pjd_batch_set_blur + pjd_blur_taps + pjd_blur_index + pjd_blur_check: every output
 *                                                       through a separable Gaussian of its own in one launch behind the resample
 *                                                       (torchvision's GaussianBlur of SimCLR, MoCo v2, BYOL, DINO, SwAV)
 *
 * Plain pointers and sizes only; no C++ or torch types.  Thread model: one
 * submitting thread per pjd_ctx (the reference has one consumer thread,
 * decoder_host.cpp:213).  All functions return 0 on success or a negative
 * PJD_E_* code; nothing here falls back to a CPU implementation -- without a
 * usable gfx950 device pjd_open fails.
 */
#ifndef PJD_H
#define PJD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever a struct in this header changes size or layout (pjd_image_desc gained qt_slot48 and
 * pjd_batch_info grew in version 2; version 3 added the coefficient download and pjd_split_*; version 4 the progressive scans of
 * pjd_image_desc and the exact-path figures of pjd_batch_info; version 5 pjd_batch_info::n_steps; version 6 the output scale
 * PJD_F_SCALE_* and pjd_pipe_opts::image_flags of pjd_pipeline.h).  PJD_OUT_RGB8_PLANAR and PJD_F_LIBJPEG changed no struct and
 * no version: a caller that needs one of them checks for it by its symbols (pjd_libjpeg_idct is exported from the first library that
 * knows PJD_F_LIBJPEG; an older one ignores the bit).  Pad on decode (pjd_batch_set_resize_pad, pjd_batch_set_pad_value) changed no
 * struct either, so PJD_VERSION stays 6: a caller checks for it by the symbol pjd_resize_pad_check.  Views (pjd_batch_set_views)
 * changed no struct: a caller checks for them by the symbol pjd_batch_n_outputs.  The affine warp (pjd_batch_set_resize_affine) changed
 * none: a caller checks for it by the symbol pjd_warp_tap.  The colour map (pjd_batch_set_colour) changed none: a caller checks for it
 * by the symbol pjd_colour_value.  The Gaussian blur (pjd_batch_set_blur) changed none: the symbol pjd_blur_taps.  pjd_batch_decode_chains changed none either: a caller checks for it by its own symbol.
 * A caller built against another version must not pass its structs: check pjd_version() == PJD_VERSION after loading.     */
#define PJD_VERSION 6

/* ---- error codes (library level) ---------------------------------------- */
#define PJD_OK              0
#define PJD_E_NODEVICE     -1   /* no HIP device / not gfx950                   */
#define PJD_E_HIP          -2   /* a HIP call failed (see pjd_last_error)       */
#define PJD_E_ARG          -3   /* bad argument / descriptor outside envelope   */
#define PJD_E_NOMEM        -4
#define PJD_E_STATE        -5   /* call order violated (e.g. decode before upload) */

/* ---- per-image status: the reference's Huffman error classes ------------- *
 * (jpeg_scanner.cpp:470-514).  As in the reference (decoder_host.cpp:181 drops
 * the bool), an image with a non-zero status still has its partial picture
 * written: everything decoded before the error, grey (128) after it.          */
#define PJD_ST_OK        0
#define PJD_ST_DC_SYM    1   /* "Error - Invalid DC value (255)"                        */
#define PJD_ST_DC_LEN    2   /* "Error - DC coefficient length greater than 11"         */
#define PJD_ST_DC_BITS   3   /* "Error - Invalid DC value"                              */
#define PJD_ST_AC_SYM    4   /* "Error - Invalid AC value"  (symbol)                    */
#define PJD_ST_AC_RUN    5   /* "Error - Zero run-length exceeded block component"      */
#define PJD_ST_AC_LEN    6   /* "Error - AC coefficient length greater than 10"         */
#define PJD_ST_AC_BITS   7   /* "Error - Invalid AC value"  (value bits)                */
/* In the branches a progressive scan takes (jpeg_scanner.cpp:521-704) the reference words some of these otherwise; the classes, and
 * the strings pjd_status_string returns, stay as above.  Message there -> class here:
 *   "Invalid DC value" (no "(255)")                 -> PJD_ST_DC_SYM (no code for the DC symbol) or PJD_ST_DC_BITS (the data ends in
 *                                                      the value bits, or before a DC refinement bit)
 *   "DC coefficient length greater than 11"         -> PJD_ST_DC_LEN
 *   "Invalid AC value"                              -> PJD_ST_AC_SYM (no code; a refinement symbol whose size is not 0 or 1) or
 *                                                      PJD_ST_AC_BITS (the data ends in value bits, in the extra bits of an end-of-band
 *                                                      run, before a sign bit or before a correction bit)
 *   "Zero run-length exceeded spectral selection"   -> PJD_ST_AC_RUN (a run or a ZRL that passes Se in an AC first scan; in a refinement
 *                                                      scan such a run is no error: the coefficient is dropped)
 *   "AC coefficient length greater than 10"         -> PJD_ST_AC_LEN
 * tests/test_progressive_streams.py checks every broken stream's reference message against this table.                              */

/* ---- output formats ------------------------------------------------------- */
#define PJD_OUT_RGB8   0   /* top-down, tightly packed R,G,B bytes: 3*W*H bytes (W, H: of the picture
                              at its output scale, PJD_F_SCALE_*)                              */
#define PJD_OUT_BMP    1   /* the complete file image bmp_writer.cpp:19-67 would emit:
                              26-byte BITMAPCOREHEADER file header, bottom-up B,G,R rows,
                              (W % 4) zero bytes after each row                               */
#define PJD_OUT_RGB8_PLANAR 2  /* planar channels, uint8[3][H][W] ("CHW"): the R plane, then the G plane, then
                              the B plane, each H top-down rows of W bytes, no padding: 3*W*H bytes (W, H
                              at the output scale).  Byte (c, y, x) is byte (y, x, c) of the PJD_OUT_RGB8
                              picture of the same descriptor; everything else (status words, partial
                              pictures, shards, coefficients) is as for PJD_OUT_RGB8.  A one-component
                              JPEG gives three equal planes.                                      */
#define PJD_OUT_GRAY8  4   /* one plane, uint8[H][W]: H top-down rows of W bytes, no padding: W*H bytes (W, H at
                              the output scale).  The luma of the picture, as libjpeg's JCS_GRAYSCALE delivers it:
                              the section "grey output" below is normative.  3 is not a format: it stays the
                              unknown value callers were promised PJD_E_ARG for (as 2 is no resize filter).     */

/* ---- descriptor flags ----------------------------------------------------- */
#define PJD_F_STANDARD_RESTART  1u  /* restart at every `restart_interval`-th MCU (ITU T.81).
                                       Default (flag clear) reproduces the reference's rule
                                       (jpeg_scanner.cpp:723), which differs -- and garbles --
                                       when luma sampling is not 1x1.                         */
#define PJD_F_FORCE_SEQUENTIAL  2u  /* decode with the one-lane exact kernel (debug/diagnosis) */
#define PJD_F_STANDARD_ZIGZAG   4u  /* zigzag slot 48 -> natural position 58 (ITU T.81) instead of
                                       the reference's 38 (common.h:16), for coefficients and for
                                       the quantiser (qt_slot48).  NOT reference-comparable: the
                                       reference has no such mode, parity for it is unpinned.   */

#define PJD_F_PROGRESSIVE       8u  /* a progressive (SOF2) frame: `scans` / `n_scans` describe its scans (at most PJD_MAX_SCANS),
                                       `ecs` is unused.  The reference cannot decode such a FILE -- its scanner stops at the first
                                       marker between scans (jpeg_scanner.cpp:425-430) -- but it carries the four procedures
                                       (decode_MCU_component, :521-704), and those are pinned: DC first, DC refinement, AC first and AC
                                       refinement with end-of-band runs, the end-of-data rule and the error class of a broken scan
                                       equal the reference's procedures run block by block on hand-built scans
                                       (tests/test_progressive_streams.py, tests/test_gpu_progressive_streams.py).  Like the
                                       reference, an AC first scan stores zeros over the slots of a run and of a ZRL (visible only
                                       where bands overlap).  NOT the reference's: the order of the blocks of a non-interleaved
                                       scan (ITU T.81 A.2.3, cross-checked against libjpeg's files), and the refinement history
                                       per zigzag slot under PJD_F_STANDARD_ZIGZAG.  Opt-in (pjd_scan_*_ex with
                                       PJD_SCAN_PROGRESSIVE), SURVEY 8(f) N4.                                                  */
#define PJD_MAX_SCANS        1024u  /* scans of one progressive frame: the scanner rejects a file with more ("Too many scans"), the
                                       planner a descriptor with more                                                          */

/* Reduced-size output, chosen per picture: s = 1 << ((flags >> 4) & 3), s = 1 (flag clear) is the full-size picture.  For s > 1,
 * with P the W x H picture the library produces at s = 1 (as RGB8: the reference's picture, or the partial picture with grey after an
 * entropy-coding error):
 *   - the output is ceil(W/s) x ceil(H/s) (libjpeg's jdiv_round_up);
 *   - output pixel (i, j) covers the source pixels x in [s*i, min(s*i + s, W)), y in [s*j, min(s*j + s, H)), n of them, and each
 *     channel is (sum + (n >> 1)) / n in integer arithmetic over their clamped 8-bit R, G, B values (boxes are partial only at the
 *     right and bottom picture edge);
 *   - PJD_OUT_RGB8 gives tight rows of 3*ceil(W/s) bytes; PJD_OUT_BMP the file the reference's BMP writer would produce for a picture
 *     of the scaled size (header with the scaled width and height, bottom-up B,G,R rows, sw % 4 zero bytes after each, sw = ceil(W/s));
 *   - the status is the one of s = 1.
 * Only the pixels change: coefficients (pjd_batch_download_coefficients) and pjd_exec_dpu_payload do not depend on the scale.  */
#define PJD_F_SCALE_1_2        16u
#define PJD_F_SCALE_1_4        32u
#define PJD_F_SCALE_1_8        48u
#define PJD_F_SCALE_MASK       48u

/* ---- libjpeg-exact decode ------------------------------------------------------------------------------------------------------ *
 * PJD_F_LIBJPEG, chosen per picture: the picture P of the descriptor is the one libjpeg (libjpeg-turbo, Pillow, torchvision.io,
 * OpenCV) decodes with its defaults -- jpeg_idct_islow, do_fancy_upsampling, the JFIF colour tables -- byte for byte, instead of the
 * reference's.  The flag implies PJD_F_STANDARD_ZIGZAG and PJD_F_STANDARD_RESTART for that picture, set or not.  Everything in this
 * header that says "the picture the library produces" then means this P: the three output formats (the BMP is the same file image built
 * from this P), the library's own buffer and pjd_batch_bind_output, pjd_batch_set_resize, _set_resize_filter, _set_resize_window,
 * _set_orientation and _set_normalize (their kernels are unchanged: they read P).  Status words are unchanged; a batch may mix flagged
 * and unflagged pictures, and the unflagged ones are decoded by the very kernels of a batch without the flag.
 *
 * THE ARITHMETIC (normative; all integers, 32-bit two's complement that WRAPS, shifts arithmetic).  Coefficients are the entropy
 * decoder's, placed through the T.81 zigzag; a unit or slot never decoded is 0 (absolute DC 0) -- every unit behind an entropy-coding
 * error included, which is what makes the partial picture grey (128) there.
 *   1. Dequantise: d[k] = coef[k] * Q[k], coef an int16, Q the 8- or 16-bit quantiser, the product in 32 bits.
 *   2. IDCT: libjpeg's jpeg_idct_islow (jidctint.c), CONST_BITS = 13, PASS1_BITS = 2.  The 1-D kernel on inputs i0..i7:
 *          z1=(i2+i6)*4433; t2=z1-i6*15137; t3=z1+i2*6270; t0=(i0+i4)<<13; t1=(i0-i4)<<13
 *          t10=t0+t3; t13=t0-t3; t11=t1+t2; t12=t1-t2
 *          a0=i7; a1=i5; a2=i3; a3=i1; z1=a0+a3; z2=a1+a2; z3=a0+a2; z4=a1+a3; z5=(z3+z4)*9633
 *          a0*=2446; a1*=16819; a2*=25172; a3*=12299; z1*=-7373; z2*=-20995; z3=z3*-16069+z5; z4=z4*-3196+z5
 *          a0+=z1+z3; a1+=z2+z4; a2+=z2+z3; a3+=z1+z4
 *          o0,o7=t10+-a3; o1,o6=t11+-a2; o2,o5=t12+-a1; o3,o4=t13+-a0;   each (o + (1<<(s-1))) >> s
 *      Pass 1 runs on the COLUMNS of d with s = 11 into a 32-bit workspace, pass 2 on the workspace's rows with s = 18; the sample is
 *      clamp(o + 128, 0, 255).  libjpeg's shortcut for a column without AC terms gives the value of the full pass (dc << 2): there is
 *      no data-dependent form.  For a stream whose dequantised values fit int16 and whose passes do not overflow -- every file an
 *      encoder made -- this is libjpeg's picture.  Beyond that it is THIS LIBRARY'S OWN deterministic definition (libjpeg masks its
 *      range-limit table where this clamps, and its behaviour on overflow is undefined C): such streams are pinned to
 *      pjd_libjpeg_idct below, not to libjpeg.
 *   3. Chroma upsampling: libjpeg's do_fancy_upsampling.  With n = ceil(W/hs) columns and m = ceil(H/vs) rows of the chroma plane
 *      (downsampled_width / _height) -- samples beyond n or m NEVER contribute, although the padded MCU holds decoded data there:
 *        hs = 2, vs = 1, n > 2:  out[2i] = (3*c[i] + c[i-1] + 1) >> 2,  out[2i+1] = (3*c[i] + c[i+1] + 2) >> 2,
 *                                except out[0] = c[0] and out[2n-1] = c[n-1]
 *        hs = vs = 2, n > 2:     for output row 2r+v the neighbour row is r-1 (v = 0) or r+1 (v = 1), clamped to 0..m-1;
 *                                s[i] = 3*c[r][i] + c[nb][i];  out[2i] = (3*s[i] + s[i-1] + 8) >> 4,  out[2i+1] = (3*s[i] + s[i+1] + 7) >> 4,
 *                                except out[0] = (4*s[0] + 8) >> 4 and out[2n-1] = (4*s[n-1] + 7) >> 4
 *        n <= 2 (pictures at most 4 wide): plain replication on both axes (libjpeg switches its fancy routines off there)
 *        hs = vs = 1, and one-component pictures: no upsampling.
 *   4. Colour: libjpeg's ycc_rgb_convert tables, 16 fraction bits.  With cb = Cb - 128, cr = Cr - 128:
 *          R = clamp(Y + ((91881*cr + 32768) >> 16))
 *          G = clamp(Y + ((-22554*cb - 46802*cr + 32768) >> 16))
 *          B = clamp(Y + ((116130*cb + 32768) >> 16))
 *      A one-component picture gives R = G = B = Y.
 * tests/test_libjpeg_cpu.py and tests/test_gpu_libjpeg.py hold this against Pillow's decode of files Pillow wrote: zero tolerance.
 * tests/test_libjpeg_corpus_cpu.py and tests/test_gpu_libjpeg_corpus.py do so on a seeded family up to libjpeg's 65500-sample limit;
 * tests/test_libjpeg_progressive_cpu.py and tests/test_gpu_libjpeg_progressive.py on progressive frames under scan scripts no encoder
 * writes (tests/golden/libjpeg_progressive/), and hold incomplete and broken progressive frames to the arithmetic above.
 *
 * ENVELOPE.  Baseline and progressive frames (with PJD_F_PROGRESSIVE Pillow's progressive files equal Pillow's decode); sampling
 * 4:4:4, 4:2:2 (h2v1), 4:2:0, or one component; the parallel path, PJD_F_FORCE_SEQUENTIAL and the exact-kernel fallback of
 * pjd_batch_sync; captured graphs.  A PROGRESSIVE frame equals libjpeg's picture only where its scans leave every coefficient fully
 * refined (each slot of each component reached by a first scan and by every refinement scan down to Al = 0), whatever the order,
 * bands, restart intervals and table ids of the scans.  Otherwise -- a scan script that stops early -- and behind an entropy-coding
 * error, P is THIS LIBRARY'S definition: the arithmetic above on the coefficients decoded so far (a slot no scan reached is 0, a slot
 * refined down to Al keeps its low Al bits zero, scans behind an error are not run).  What is not reproduced is libjpeg's interblock
 * smoothing (jdcoefct.c, do_block_smoothing), which it applies to a progressive frame whose coefficients are not fully refined: on
 * five pictures of tests/golden/libjpeg_progressive/ rewritten without their last four scans Pillow's decode lies 19, 10, 3, 3 and 2
 * levels from P (136 x 72 4:2:0 q50, 259 x 19 4:2:2 q75, 40 x 24 4:4:4 q95, 33 x 31 grey q85, 61 x 45 4:2:0 q90; the complete files:
 * 0).  pjd_batch_create returns PJD_E_ARG (pjd_last_error names the picture) for the flag together with
 * PJD_F_SCALE_* (libjpeg's reduced IDCTs are other filters), with 4:4:0 (h1v2) sampling, with two components, or on a shard
 * (so pjd_split_decode refuses a flagged descriptor too).  pjd_batch_download_coefficients returns the coefficients as under
 * PJD_F_STANDARD_ZIGZAG.
 * HOW.  Two more launches for the flagged pictures of a batch (pjd_batch_decode_timed names them "idct_std" and "colour_std"; part of
 * a captured graph; run again after the exact-kernel fallback): the IDCT into uint8 component planes -- an intermediate buffer of the
 * batch, whole MCUs per picture, counted in pjd_batch_info::device_bytes, every byte written by every decode -- then upsampling,
 * colour and the store into exactly the ranges the default back end writes.  A batch that holds a flagged picture is decoded as one
 * chain of launches.  A batch without one allocates and launches nothing new.
 * The three functions below are the arithmetic on its own, host only (no device needed), the very inlines the kernels run:
 * pjd_libjpeg_idct steps 1 and 2 for one unit (coef, q and out in natural order); pjd_libjpeg_ycc_to_rgb step 4 for one pixel;
 * pjd_libjpeg_upsample_row step 3 for one output row: `cur` is the chroma row c[r] and `nb` its neighbour row c[nb] (NULL: h2v1; `v`
 * says which neighbour it is, and changes nothing), n samples each, and out receives 2n samples.  PJD_E_ARG for a null pointer or
 * n = 0.                                                                                                                          */
#define PJD_F_LIBJPEG          64u
int  pjd_libjpeg_idct(const int16_t coef[64], const uint16_t q[64], uint8_t out[64]);            /* host only, no device needed */
int  pjd_libjpeg_ycc_to_rgb(uint8_t y, uint8_t cb, uint8_t cr, uint8_t rgb[3]);                /* host only, no device needed */
int  pjd_libjpeg_upsample_row(const uint8_t *cur, const uint8_t *nb, int v, uint32_t n, uint8_t *out /* 2n */);   /* host only */

/* ---- libjpeg-exact REDUCED-SIZE decode ------------------------------------------------------------------------------------------- *
 * PJD_F_LIBJPEG_SCALE_*, per picture, only together with PJD_F_LIBJPEG: the picture P is the one libjpeg decodes with scale_num /
 * scale_denom = 1/s, s = 2, 4 or 8 -- Pillow's Image.draft() and thumbnail(), OpenCV's IMREAD_REDUCED_*, draft-before-resize loaders
 * -- through its reduced IDCTs (jidctred.c), byte for byte.  P is ceil(W/s) x ceil(H/s); pjd_scaled_dims, pjd_image_output_size,
 * pjd_batch_output_size and the BMP header give that size, and everything downstream (resize filters, windows, orientation, pad,
 * normalised output, bound output) reads this P.  These are bits of their own: PJD_F_SCALE_* stays the box filter, which is not what
 * libjpeg does, and stays refused together with PJD_F_LIBJPEG.
 *
 * THE ARITHMETIC (normative; 32-bit two's complement that WRAPS, shifts arithmetic; coefficients, d[k] = coef[k] * Q[k], the zigzag and
 * "never decoded is 0" as in the section above).  Let n = 8/s.
 *   SIZES (libjpeg jdmaster.c).  A luma unit becomes n x n samples.  A chroma unit becomes cn x cn: cn starts at n and doubles while
 *   cn < 8, 2*cn <= hs*n and 2*cn <= vs*n.  So 4:4:4 and one component: cn = n.  4:2:2 (h2v1): cn = n, the h2v1 upsampling remains.
 *   4:2:0: cn = 2n and NO upsampling is left -- at 1/2 the chroma units go through the full jpeg_idct_islow, at 1/4 through the 4x4
 *   transform, at 1/8 through the 2x2 one.
 *   TRANSFORMS (libjpeg jidctred.c).  Each output o is (o + (1 << (sh-1))) >> sh; the sample is clamp(o + 128, 0, 255).  No
 *   data-dependent form: libjpeg's DC-only shortcut gives the value of the full pass.
 *     8x8  as in the section above.
 *     4x4  the 1-D kernel reads i0, i1, i2, i3, i5, i6, i7 (input 4 is never read):
 *              t0 = i0 << 14;  t2 = i2*15137 - i6*6270;  t10 = t0 + t2;  t12 = t0 - t2
 *              a0 = -i7*1730 + i5*11893 - i3*17799 + i1*8697
 *              a2 = -i7*4176 - i5*4926  + i3*7373  + i1*20995
 *              o0 = t10 + a2;  o1 = t12 + a0;  o2 = t12 - a0;  o3 = t10 - a2
 *          Pass 1 runs on columns 0, 1, 2, 3, 5, 6, 7 of d (rows as inputs) with sh = 12 into a workspace of 4 rows x 8 columns; pass 2
 *          on each of the 4 workspace rows, reading columns 0, 1, 2, 3, 5, 6, 7, with sh = 19.
 *     2x2  the 1-D kernel reads i0, i1, i3, i5, i7:
 *              t10 = i0 << 15;  t0 = -i7*5906 + i5*6967 - i3*10426 + i1*29692;  o0 = t10 + t0;  o1 = t10 - t0
 *          Pass 1 runs on columns 0, 1, 3, 5, 7 with sh = 13; pass 2 on the 2 workspace rows over the same columns with sh = 20.
 *     1x1  clamp(((d[0] + 4) >> 3) + 128, 0, 255).
 *   UPSAMPLING.  Only 4:2:2 has any left.  The chroma plane has dw = ceil(W*cn/16) columns and dh = ceil(H*cn/8) rows that belong to
 *   the picture; samples beyond them never contribute.  Where n > 1 and dw > 2 it is the h2v1 fancy rule of step 3 above; at 1/8
 *   (n = 1: libjpeg switches fancy upsampling off when min_DCT_scaled_size is 1) and where dw <= 2 it is plain replication.
 *   COLOUR.  Step 4 above, unchanged.
 *   GREY (PJD_OUT_GRAY8): the luma plane at n x n per unit -- what draft("L", ...) delivers.
 *   Behind an entropy-coding error every sample is 128 at every scale.  For streams whose values overflow the caveat of the full-size
 *   section holds: this text, not libjpeg, is the definition.
 * VERIFIED on the CPU against Pillow 12.2.0 (libjpeg-turbo) with a numpy model of this text fed the oracle port's coefficients: 16
 * sizes from 1x1 to 259x19, 4:4:4, 4:2:2, 4:2:0 and one component, q 50 / 90 / 100, scales 1/1 .. 1/8, RGB and draft("L") of colour
 * files: 672 decodes each way, zero differing bytes.  tests/test_libjpeg_scaled_cpu.py and tests/test_gpu_libjpeg_scaled.py hold the
 * model, the export below and the kernels against Pillow's recorded draft decodes (tests/golden/libjpeg_scaled/): zero tolerance.
 *
 * ENVELOPE.  That of PJD_F_LIBJPEG (no 4:4:0, no two components, no shard).  pjd_batch_create / pjd_plan_check return PJD_E_ARG, the
 * picture named, for one of these bits without PJD_F_LIBJPEG and for one together with PJD_F_SCALE_*.  A batch may mix flagged
 * pictures at any of the four scales with unflagged pictures, box-scaled or not; the unflagged ones and the full-size flagged ones
 * keep the very kernels they have without this feature.  Coefficients and status words do not depend on the scale.
 * HOW.  The reduced pictures' ranges go through kernels of their own in the same two launches' places (timed under the same names
 * "idct_std", "colour_std", "idct_gray_std"): pass 1 only on the columns a transform reads, a unit row's n samples as one store, the
 * component planes at the reduced geometry (luma mcux*hs*n x mcuy*vs*n, chroma mcux*cn x mcuy*cn: device_bytes shrinks with them).
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for the symbol pjd_libjpeg_idct_scaled -- the inline the
 * kernels run, host only: n x n samples of one unit for n = 8, 4, 2 or 1 (coef and q in natural order), PJD_E_ARG for any other n or a
 * null pointer.  An older library ignores the bits and returns full-size pictures.                                                    */
#define PJD_F_LIBJPEG_SCALE_1_2   128u
#define PJD_F_LIBJPEG_SCALE_1_4   256u
#define PJD_F_LIBJPEG_SCALE_1_8   384u
#define PJD_F_LIBJPEG_SCALE_MASK  384u
int  pjd_libjpeg_idct_scaled(const int16_t coef[64], const uint16_t q[64], uint32_t n, uint8_t *out /* n*n */);   /* host only */

/* ---- grey output ----------------------------------------------------------------------------------------------------------------- *
 * PJD_OUT_GRAY8, chosen per batch: every picture leaves as ONE plane, uint8[H][W], top-down, tight rows, W*H bytes, W and H at the
 * picture's output scale -- what torchvision.io.decode_jpeg(mode=GRAY), OpenCV's IMREAD_GRAYSCALE and Pillow's draft("L") deliver.
 *
 * DEFINITION (normative).  Let P0 be the picture the library would produce for the descriptor if every chroma sample were neutral:
 * Cb = Cr = 0 after the IDCT under the reference's arithmetic, Cb = Cr = 128 under PJD_F_LIBJPEG.  Then R = G = B in P0, and byte
 * (y, x) of the PJD_OUT_GRAY8 picture is that common value:
 *   - under the reference's arithmetic clamp255(Y + 128), Y the int16 luma sample after the reference's IDCT (dequantisation, the
 *     zigzag quirk and its slot-52 rule included): src/decoder_dpu.c:376-382 with both chroma terms zero;
 *   - under PJD_F_LIBJPEG libjpeg's own luma sample, steps 1 and 2 of that section -- what libjpeg delivers with out_color_space =
 *     JCS_GRAYSCALE.  It is NOT a weighted sum of the clamped R, G and B of the colour picture (Pillow's convert("L") of its RGB
 *     decode is up to 24 levels away on the fixtures of tests/golden/libjpeg/); tests/golden/libjpeg_gray/ holds Pillow's draft("L").
 * A one-component JPEG gives the plane its three equal RGB planes are.  After an entropy-coding error the undecoded part is 128.
 * Status words, coefficients (pjd_batch_download_coefficients), every figure of pjd_plan_info but the byte counts, lane planning and
 * the entropy decoder are those of any other format: only the back end differs.
 * WITH PJD_F_SCALE_*: the box filter of that section on the one plane -- channel 0 of what it makes of P0.
 * SIZES.  pjd_output_size, pjd_image_output_size and pjd_batch_output_size give W*H; pictures in the library's own buffer stay
 * 256-byte aligned (pjd_batch_output_offset, pjd_batch_download_packed: a third of the bytes of an RGB batch over the host link);
 * pjd_batch_bind_output takes the batch as it takes a planar one and promises no alignment; every decode writes every byte of every
 * unsharded picture's range and no byte outside it; a shard (shard_n_segs != 0) is accepted as in a PJD_OUT_RGB8 batch and only its
 * MCUs are written.  pjd_batch_capture, the exact-kernel fallback of pjd_batch_sync, pjd_decode_batch, pjd_plan_check and
 * pjd_pipe_opts::out_format (the sink receives W*H bytes) take the format.
 * EVERYTHING DOWNSTREAM is channel 0 of what the three-channel pipeline would do to P0; no filter has arithmetic of its own.  A grey
 * batch is a planar batch with ONE plane: pjd_batch_set_resize, _set_resize_filter (all three filters), _set_resize_window,
 * _set_orientation and _set_resize_pad keep their rules, call order and errors, and pjd_batch_output_size is tw*th (times the element
 * size when normalised).  pjd_batch_set_normalize: fma(v, scale[0], bias[0]); all six constants are still validated as finite, entries
 * [1] and [2] are ignored.  pjd_batch_set_resize_pad / _set_pad_value: fill[0] and value[0].  pjd_batch_bind_output of a normalised
 * batch wants element alignment, as for the other formats.
 * REFUSED with PJD_E_ARG: pjd_split_decode with this format; everything a planar batch refuses (a resize or a normalisation of a
 * shard, targets outside 1..65535, a picture more than 16x its target under a table-driven filter, ...); PJD_F_LIBJPEG together with
 * PJD_F_SCALE_*, 4:4:0 sampling, two components or a shard, exactly as in the other formats.
 * HOW.  Kernels of their own (pjd_k_backend_gray.hip; pjd_batch_decode_timed names them "idct_gray" and, for the flagged pictures of a
 * batch, "idct_gray_std"): the entropy decoder's streams interleave the components, so chroma entries are still walked, but chroma
 * units are not dequantised, not DC-settled and not transformed; there is no upsampling and no colour arithmetic, and a lane stores
 * eight adjacent pixels at once.  A flagged picture's luma rows go straight from the islow IDCT into the picture: a grey batch has no
 * component planes (pjd_batch_info::device_bytes) and no "colour_std" launch.  The resample of a grey batch always runs the padded
 * (most general) kernel form, with the identity window, orientation 1 and an all-zero pad where none was asked for: one channel is
 * built for that form alone.  pjd_batch_decode_timed therefore lists "pad" behind "resize" for every resized grey batch; the border
 * launch is skipped where no picture has a border.
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for pjd_output_channels (below).                          */

/* Huffman table as the reference's scanner holds it (jpeg.h:129-134):
 * offsets[k] = number of codes of length <= k (offsets[0] = 0).               */
typedef struct pjd_huff_table {
    uint8_t offsets[17];
    uint8_t symbols[162];
    uint8_t set;
} pjd_huff_table;

/* One scan of a progressive frame (ITU T.81 G.1; the fields the reference's progressive branches read from `Header`:
 * start_of_selection, end_of_selection, successive_approximation_high / _low, jpeg.h:160-163) with the Huffman tables in
 * force when the scan starts (tables may be redefined between scans) and its own entropy-coded bytes.                     */
typedef struct pjd_scan_desc {
    uint8_t  n_comp;                   /* components in this scan, 1..3 (AC scans: 1)                          */
    uint8_t  comp[3];                  /* their indices 0..2 (frame order)                                     */
    uint8_t  ss, se, ah, al;           /* spectral selection, successive approximation                         */
    uint32_t restart_interval;         /* DRI in force for this scan, in MCUs OF THE SCAN; 0 = none            */
    pjd_huff_table table[3];           /* per scan component: its DC table (ss == 0) or its AC table (ss > 0)   */
    const uint8_t *ecs;                /* destuffed, RSTn removed                                              */
    uint64_t ecs_len;
} pjd_scan_desc;

/* One parsed baseline JPEG -- exactly the fields of the reference `Header`
 * (jpeg.h:146-179) that its hot path consumes, plus the restart-segment
 * offsets the reference's scanner throws away.                                */
typedef struct pjd_image_desc {
    uint32_t width, height;            /* pixels                                              */
    uint8_t  num_components;           /* 1..3                                                */
    uint8_t  h_samp, v_samp;           /* luma sampling factors, each 1 or 2                  */
    uint8_t  comp_h[3], comp_v[3];     /* per component (chroma must be 1x1)                  */
    uint8_t  comp_qt[3], comp_dc[3], comp_ac[3];   /* table selectors, each 0..3              */
    uint8_t  qt_set[4];
    uint32_t qt[4][64];                /* NATURAL order as filled through the reference's
                                          zigzag_map (common.h:9-18, entry 48 = 38)           */
    pjd_huff_table dc[4], ac[4];
    uint32_t restart_interval;         /* DRI value, 0 = none                                 */
    const uint8_t *ecs;                /* entropy-coded bytes, destuffed (FF00 -> FF) and with
                                          RSTn removed == Header::huffman_data (jpeg.h:168)   */
    uint64_t ecs_len;                  /* below 2^29 (512 MiB: the decoder's bit positions are
                                          32-bit); 2^29 and more is refused with PJD_E_ARG.
                                          tests/test_giant_cpu.py pins the refusal on both sides,
                                          tests/test_gpu_giant.py decodes 2^29 - 1 bytes        */
    const uint64_t *seg_offsets;       /* byte offset in `ecs` of each restart segment,
                                          seg_offsets[0] == 0; NULL => one segment            */
    uint32_t n_segments;
    uint32_t flags;                    /* PJD_F_*                                             */
    /* Sharding of ONE image over several devices (restart segments are
     * independent): decode only segments [shard_first_seg, +shard_n_segs);
     * shard_n_segs == 0 means "all".  The output buffer is always the whole picture (at its output scale);
     * only the MCUs of the selected segments are written.                      */
    uint32_t shard_first_seg, shard_n_segs;
    uint32_t qt_slot48[4];             /* DQT entry 48 of each table: the reference's map sends it
                                          to natural 38, where entry 52 overwrites it, so `qt`
                                          does not hold it.  Read only with PJD_F_STANDARD_ZIGZAG. */
    const pjd_scan_desc *scans;        /* PJD_F_PROGRESSIVE only: the frame's scans in file order    */
    uint32_t n_scans;
    uint32_t reserved_;
} pjd_image_desc;

typedef struct pjd_ctx pjd_ctx;
typedef struct pjd_batch pjd_batch;

/* Kernel-level timing of one decode, HIP events on the context's stream.     */
#define PJD_MAX_KERNELS 16
typedef struct pjd_timings {
    int32_t n;
    float   ms[PJD_MAX_KERNELS];
    char    name[PJD_MAX_KERNELS][32];
    float   total_ms;                  /* first-start .. last-stop                            */
} pjd_timings;

typedef struct pjd_batch_info {
    int32_t  n_images;
    uint64_t pixels;                   /* sum of width*height of the SOURCE pictures (the decode work, whatever the scale) */
    uint64_t ecs_bytes;                /* sum of ecs_len                                      */
    uint64_t out_bytes;                /* sum of output sizes, each at the picture's output scale (PJD_F_SCALE_*), or resized (pjd_batch_set_resize), in the elements of pjd_batch_set_normalize */
    uint64_t coef_bytes;               /* lane streams + transposed bitstream words + dense scratch in HBM */
    uint64_t n_data_units;
    uint64_t n_subsequences;           /* Huffman decode lanes                                */
    uint64_t device_bytes;             /* everything this batch holds in HBM (the output buffer at the scaled sizes) */
    int32_t  n_sequential;             /* images routed to the exact one-lane kernel up front */
    int32_t  n_fallback;               /* images re-decoded by it after the last decode       */
    uint64_t n_huff_workgroups;        /* Huffman workgroups (up to 2 waves of 64 lanes, one table set) */
    /* diagnostics of the last decode: self-synchronisation effort                           */
    uint64_t sync_rounds;              /* re-sync rounds summed over workgroups               */
    uint64_t sync_lane_passes;         /* lanes that re-decoded their subsequence, summed     */
    uint64_t fix_rounds, fix_lane_passes;   /* the same for the boundary-stitch stage          */
    uint32_t sub_bytes;                /* bytes of bitstream per Huffman lane chosen for this batch */
    uint32_t n_table_sets;             /* distinct Huffman table sets (images with identical tables share one) */
    uint64_t n_huff_waves;
    uint64_t n_entries;                /* 16-bit coefficient entries (= Huffman symbols) emitted by the last decode */
    float    exact_fallback_ms;        /* GPU time (HIP events) the exact one-lane kernel + its back end took to re-decode the
                                          pictures the parallel decoder could not resolve in the last decode; 0 if none.  The exact
                                          kernel is a single dependent chain per picture: about 10 MPix/s per picture */
    uint32_t n_entropy_errors;         /* pictures of the last decode with an entropy-coding error (status != 0) that the parallel
                                          decoder settled itself                                                               */
    uint64_t flag_waves[8];            /* waves that reported something unresolved in the last decode, by reason:
                                          0 invalid symbol, 1 irregular segment end / phase, 2 re-sync did not converge,
                                          3 wave boundary did not stitch, 4 wait timed out, 5 lane output overflow,
                                          6 write pass did not reproduce the synchronised state                     */
    uint32_t huff_lds_bytes;           /* LDS of one entropy-decode workgroup: the largest table set of the batch + wave areas   */
    uint32_t plan_mode;                /* PJD_PLAN_* the batch was planned with                                                    */
    uint64_t walks, walk_lanes;        /* last decode: re-sync rounds that a wave finished as a cooperative walk (few lanes left: the
                                          whole wave decodes one lane's subsequence several times faster), and the lanes walked */
    uint64_t n_steps;                  /* last decode: steps of the write pass (a step emits one entry, or the two entries of a symbol
                                          pair that one table lookup yields): n_entries / n_steps = symbols per step               */
    uint32_t lane_fill_x1024;          /* last decode: the fullest lane region, slots written x 1024 / its capacity (capacities are a
                                          bound computed from the picture's Huffman tables: never above 1024)                    */
    uint32_t dc_plan;                  /* how the plan settles DC prediction across lanes.  Bits 0..7: the single chain's form, 0 the
                                          batch-wide scan of three launches, 1 one workgroup per picture.  Bits 8..15: the picture
                                          groups planned for an idle device (each settles its own pictures, one workgroup each), 0 if none */
} pjd_batch_info;

/* ---- context --------------------------------------------------------------- */
int  pjd_version(void);
int  pjd_open(int device_ordinal, pjd_ctx **out);
void pjd_close(pjd_ctx *ctx);
/* How batches created on this context from now on are planned.  The entropy decoder cuts every bitstream into lanes; short lanes
 * finish ONE batch sooner (every pass of every chain is shorter), long lanes cost less work per byte (fewer re-synchronisation
 * passes), which is what counts when several batches are decoded at once (pjd_pipeline, a serving loop).  Measured on the default
 * workload of bench.py: latency plan 2.15 ms for a batch alone / 121 GPix/s with four in flight, throughput plan 2.50 ms / 130.
 * Pictures are identical either way.  Default: PJD_PLAN_LATENCY (PJD_PLAN_MODE=throughput in the environment changes it).      */
#define PJD_PLAN_LATENCY     0
#define PJD_PLAN_THROUGHPUT  1
int  pjd_set_plan_mode(pjd_ctx *ctx, int mode);
const char *pjd_last_error(pjd_ctx *ctx);   /* text of the last failure on this context       */
const char *pjd_status_string(int status);  /* the reference's message for a PJD_ST_* value   */
void *pjd_stream(pjd_ctx *ctx);             /* the hipStream_t all work is issued on          */

/* ---- batch life cycle ------------------------------------------------------- *
 * create : plan + allocate (host pinned staging and HBM); copies the descriptors,
 *          the caller's ecs buffers may be released after pjd_batch_upload returns.
 * upload : H2D of bitstreams, tables and work lists, then -- once per upload, not per
 *          decode -- the kernels that build the decode tables and the entropy
 *          decoder's word rows from them (all asynchronous on the stream).
 * decode : enqueue the kernels; inputs and outputs stay resident in HBM.
 * download: D2H of pictures and statuses into caller memory, synchronises.
 * A batch can be decoded any number of times after one upload.                 */
int  pjd_batch_create(pjd_ctx *ctx, const pjd_image_desc *images, int n_images,
                      int out_format, pjd_batch **out);
int  pjd_batch_upload(pjd_batch *b);
int  pjd_batch_decode(pjd_batch *b);
int  pjd_batch_decode_timed(pjd_batch *b, pjd_timings *t);   /* same work, events per kernel  */
int  pjd_batch_capture(pjd_batch *b);       /* record the decode as a hipGraph; later
                                               pjd_batch_decode calls replay it               */
int  pjd_batch_sync(pjd_batch *b);
/* The form the LAST decode of the batch was issued in: 0 before the first one, 1 for one chain of launches, g >= 2 for the chains of
 * g picture groups on streams of their own (what a batch of 64 or more small pictures takes when no other grouped decode is in flight
 * on the device; PJD_IDLE_FORM=chain turns it off).  What was issued, not what the planner made (pjd_batch_info.dc_plan >> 8): 1 where
 * the group streams could not be had, 1 for every pjd_batch_decode_timed, and for a replay the form of the graph that was launched.
 * pjd_batch_capture and the exact-kernel fallback of pjd_batch_sync leave it alone.  PJD_E_ARG for NULL.  Host only.             */
int  pjd_batch_decode_chains(pjd_batch *b);
int  pjd_batch_download(pjd_batch *b, uint8_t *const *out, int32_t *status);
/* All pictures in ONE device-to-host copy: `host` receives the batch's output buffer as it lies
 * in HBM (picture i at pjd_batch_output_offset(b, i), 256-byte aligned, pjd_batch_packed_size(b)
 * bytes in total).  Give it memory from pjd_host_alloc for a full-rate PCIe transfer.  This is the
 * copy(batch.mcus, "mcus") of decoder_host.cpp:308 for a whole batch.                           */
int  pjd_batch_download_packed(pjd_batch *b, uint8_t *host, uint64_t capacity, int32_t *status);
uint64_t pjd_batch_packed_size(pjd_batch *b);
uint64_t pjd_batch_output_offset(pjd_batch *b, int image);
/* After pjd_batch_create and before the first pjd_batch_upload / _capture / _decode of this batch (else PJD_E_STATE):
 * pictures are written into caller-owned device memory instead of a buffer of the batch.  Picture i occupies
 * [base + offsets[i], + pjd_batch_output_size(b, i)); offsets == NULL means the packed layout (pjd_batch_output_offset as
 * reported before the call).  No alignment is required of base or of any offset (a normalised batch: element alignment, below).
 * PJD_E_ARG for a PJD_OUT_BMP batch (its row padding relies on the library zeroing its own buffer), a pointer that is not
 * device memory of the context's device, a `capacity` that reaches past the end of the allocation the pointer lies in (where the
 * runtime can tell), a picture range that ends beyond `capacity`, two picture ranges that overlap.
 * The batch's own output buffer goes back to the context's pool (pjd_batch_info::device_bytes shrinks by its size).  The
 * library never frees, zeroes or reads the caller's memory: it writes pictures into it -- no byte outside the picture ranges,
 * and every decode writes every byte of every unsharded picture's range, so the memory may be recycled between decodes -- and
 * copies from it in pjd_batch_download.  pjd_batch_device_output / pjd_batch_output_offset report the bound addresses /
 * offsets; pjd_batch_download_packed works with the packed layout only (explicit offsets: PJD_E_STATE); a captured graph
 * records the bound addresses.  Work is issued on pjd_stream(ctx) as always, a stream without implicit order to any other: the
 * caller orders its own streams against it, both ways.  Before upload / decode: whatever still reads or writes the memory on the
 * caller's streams must have finished (or pjd_stream(ctx) made to wait for it).  After a decode: pjd_batch_sync (or a download)
 * before the pictures are read or the memory reused -- only there are the status words read back and the pictures the parallel
 * decoder gave up on decoded again by the exact kernel (pjd_batch_info::n_fallback), into the same memory.  An event recorded on
 * pjd_stream(ctx) after pjd_batch_decode orders the kernels of that decode alone: it is enough only for a batch whose decodes
 * need no such fallback (n_fallback == 0, e.g. known from an earlier pjd_batch_sync of the same batch).
 * Where the memory comes from a sub-allocator (torch's caching allocator), "the allocation" above is the allocator's whole
 * segment: that check catches a wild capacity, it does not prove that the range is the caller's own tensor.                    */
int  pjd_batch_bind_output(pjd_batch *b, void *device_base, uint64_t capacity, const uint64_t *offsets);
/* ---- resize on decode ------------------------------------------------------------------------------------------------------ *
 * pjd_batch_set_resize: picture i of the batch leaves the decode as out_w[i] x out_h[i] pixels (n_images entries each), whatever its
 * own size: a ragged batch becomes pictures of one size, i.e. one uint8[N][3][H][W] tensor when bound at offsets i * 3 * H * W.
 *
 * THE ARITHMETIC (normative).  Let P be the sw x sh picture the library produces for the descriptor without this call -- the
 * reference's picture, or the partial picture with grey after an entropy-coding error, box-filtered if PJD_F_SCALE_* is set -- and
 * its 8-bit R, G, B the source.  For a target of tw x th each axis is handled on its own: with sn source samples, dn target samples
 * and the target index i (integer arithmetic, divisions round down):
 *     X  = (2*i + 1)*sn - dn                     (64-bit; this is 2*dn*((i + 0.5)*sn/dn - 0.5))
 *     X  = clamp(X, 0, 2*dn*(sn - 1))
 *     i0 = X / (2*dn)
 *     w  = ((X - i0*2*dn)*256 + dn) / (2*dn)     (0..256)
 *     i1 = min(i0 + 1, sn - 1)
 * and per channel, with (x0, x1, wx) for the column and (y0, y1, wy) for the row of the target pixel:
 *     out = ((256-wy)*((256-wx)*P[y0][x0] + wx*P[y0][x1]) + wy*((256-wx)*P[y1][x0] + wx*P[y1][x1]) + 32768) >> 16
 * This is the bilinear filter with half-pixel centres -- torch.nn.functional.interpolate(mode="bilinear", align_corners=False,
 * antialias=False) -- with the weights quantised to 1/256 and ONE rounding: it differs from that filter computed in float64 and
 * rounded to nearest by at most 1 level (each quantised weight is off by at most 1/512: under 0.4981 levels per axis, under 0.9962
 * before the one rounding).  Every intermediate fits 24 bits (at most 16 744 448).  A target equal to the source size reproduces P
 * byte for byte (every w is 0).  pjd_resize_tap is the tap computation on its own, host only (no device needed), and the very
 * code the kernel runs: PJD_E_ARG if src_n or dst_n is 0 or above 65535 or i >= dst_n; i0, i1, w may each be NULL.  Where
 * src_n * dst_n reaches 2^31 the taps are computed in 64-bit arithmetic: tests/test_gpu_geometry.py pins that branch on the device
 * (sources and targets 65535 samples long), tests/test_geometry_cpu.py on the host.
 * ADVICE: plain bilinear aliases when it shrinks by more than about 2x per axis.  Pre-scale with PJD_F_SCALE_*: choose the largest
 * s of 1, 2, 4, 8 with ceil(W/s) >= tw and ceil(H/s) >= th (the box filter takes the bulk of the reduction, and less is decoded);
 * the bilinear step then shrinks by less than 2x on the axis that limits s (on both where picture and target have one aspect ratio;
 * beyond s = 8 nothing is left to take, and the other axis of a picture squeezed out of shape keeps its larger factor).  What the
 * pre-scale leaves, pjd_batch_set_resize_filter(b, PJD_RESIZE_ANTIALIAS) removes: the antialiased filter below.
 *
 * CALL ORDER.  After pjd_batch_create and before any pjd_batch_bind_output / _upload / _capture / _decode of the batch, once:
 * PJD_E_STATE otherwise.  PJD_E_ARG (pjd_last_error names the picture) for a null array, a target dimension of 0 or above 65535,
 * a PJD_OUT_BMP batch, a batch that holds a shard (shard_n_segs != 0: a shard's picture is only partly written).
 * FROM THEN ON pjd_batch_output_size(b, i) is 3 * out_w[i] * out_h[i]; pjd_batch_output_offset, _packed_size, _device_output,
 * _download, _download_packed and _bind_output speak about the resized pictures (offsets in the library's own buffer stay 256-byte
 * aligned; bind_output checks its ranges against the resized sizes and promises no alignment, as before).  PJD_OUT_RGB8_PLANAR gives
 * uint8[3][th][tw], PJD_OUT_RGB8 tight rows of 3 * tw bytes.  Every decode writes every byte of every picture's range and no byte
 * outside it.  The picture at its decode size lives in an intermediate buffer of the batch (in the batch's output format; counted in
 * pjd_batch_info::device_bytes, and not given up by pjd_batch_bind_output, which redirects the resized pictures alone);
 * pjd_batch_info::out_bytes is the sum of the resized sizes, `pixels` stays the source pixels.  The resample is one more launch on
 * pjd_stream(ctx) behind the back end of every decode (part of a captured graph; pjd_batch_decode_timed names it "resize"), and
 * runs again after the exact-kernel fallback of pjd_batch_sync.  Status words, coefficients (pjd_batch_download_coefficients) and
 * pjd_plan_info are unaffected.                                                                                                  */
int  pjd_batch_set_resize(pjd_batch *b, const uint32_t *out_w, const uint32_t *out_h);
int  pjd_resize_tap(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *i0, uint32_t *i1, uint32_t *w);
/* ---- antialiased resize ------------------------------------------------------------------------------------------------------ *
 * pjd_batch_set_resize_filter(b, PJD_RESIZE_ANTIALIAS): the resize of the batch uses the triangle filter WIDENED where an axis
 * shrinks -- torch.nn.functional.interpolate(mode="bilinear", antialias=True), Pillow's BILINEAR -- instead of the plain bilinear
 * one above.  PJD_RESIZE_BILINEAR (and no call at all) leaves everything as described above;
 * PJD_RESIZE_BICUBIC is specified further down.
 *
 * THE ARITHMETIC (normative).  The source P is the source of pjd_batch_set_resize: the picture at its decode size, after
 * PJD_F_SCALE_*, with grey after an entropy-coding error.  Each axis is handled on its own.  Per axis, with sn source samples, dn
 * target samples, the target index i and S = max(sn, dn) (integer arithmetic, 64-bit where needed, divisions round down):
 *     r_j = max(0, 2*S - |(2*j + 1)*dn - (2*i + 1)*sn|)       raw weight of source sample j, 0 <= j < sn
 * the triangle with half-pixel centres, of half-width 1 target sample where the axis grows or stays (bilinear) and of half-width
 * sn/dn source samples where it shrinks; samples outside the picture are dropped and the rest renormalised, as Pillow and torch
 * do.  The TAPS are the contiguous run of j with r_j > 0: `first`, `count`, and R = sum r_j.  Quantised to 1/65536:
 *     q_j = (r_j*65536 + R/2) / R
 * and then 65536 - sum q_j is added to the tap with the largest r_j (the lowest j on a tie), so that sum q_j == 65536 exactly.
 * Every q_j lies in 0..65536; a single tap has q = 65536 (17 bits).  Per channel, with (first, count, qx) of the target column and
 * (first, count, qy) of the target row:
 *     h   = sum_x qx * P[y][x]                   (at most 65536 * 255, below 2^24)
 *     h16 = (h + 128) >> 8                       (the row sample with 8 fraction bits, at most 65280)
 *     v   = sum_y qy * h16                       (at most 65536 * 65280: v + 2^23 fits 32 bits)
 *     out = (v + (1 << 23)) >> 24
 * Every product has operands of at most 24 bits.  Where dn == sn the only tap is j == i with q = 65536: a target equal to the
 * source size reproduces P byte for byte, and a constant picture stays constant (the weights sum to 65536 exactly).
 * ERROR BOUND.  A rounded q_j is within 1/2 of r_j*65536/R, so the sum of the n rounded taps is within n/2 of 65536, and the
 * correction moves one tap by at most n/2: the absolute errors of an axis' weights sum to at most n/65536 of a weight, i.e. at most
 * 255*n/65536 levels per axis -- 0.1246 at the n = 32 of the limit below.  The horizontal error passes through the vertical pass
 * with weights that sum to 1, h16 adds its rounding (1/512 level), the vertical weights their own 0.1246: under 0.252 levels from the
 * exact filter before the ONE final rounding, which adds at most 1/2.  The result therefore differs from the filter computed in
 * float64 and rounded to nearest by at most 1 level (measured: under 0.503 before rounding, tests/test_resize_aa_cpu.py).
 * LIMIT.  sn <= 16*dn on each axis, at the decode size (with the 1/8 pre-scale of PJD_F_SCALE_* in front: 128x in all).
 * PJD_AA_MAX_TAPS is the largest tap count the limit admits: the taps are the j with (2*j + 1)*dn inside an OPEN interval of length
 * 4*S around (2*i + 1)*sn; the points are 2*dn apart, and an open interval of length L holds at most ceil(L / d) points d apart:
 * ceil(2*S/dn) -- 2 where the axis grows, at most 32 where sn <= 16*dn, attained by 64 -> 4.  (33 would need the closed interval.)
 *
 * CALL ORDER.  After pjd_batch_set_resize; before any pjd_batch_set_normalize / _bind_output / _upload / _capture / _decode of the
 * batch; once: PJD_E_STATE otherwise, also when no resize is set.  PJD_E_ARG for an unknown filter, or (PJD_RESIZE_ANTIALIAS) for
 * a picture whose decode size exceeds 16x its target on an axis (pjd_last_error names the picture); where the batch has source
 * windows (pjd_batch_set_resize_window, below) the limit is each window's against its virtual target, and the weights are those of
 * the windowed axes.
 * FROM THEN ON everything pjd_batch_set_resize promises from its "FROM THEN ON" holds unchanged -- sizes, offsets, bind_output,
 * downloads, every byte of every range written and none outside, the one launch named "resize", part of a captured graph, run again
 * after the exact-kernel fallback -- and pjd_batch_set_normalize composes with it as with the bilinear filter: the fma and the
 * conversion are applied to `out`.  The weights are computed once, by this call, into a table of the batch (shared between
 * pictures with the same source and target length on an axis; counted in pjd_batch_info::device_bytes, sent by pjd_batch_upload).
 * pjd_resize_aa_taps is the tap computation on its own, host only (no device needed), the very inline the table is built with:
 * first, count and q[0 .. count-1] (q has room for PJD_AA_MAX_TAPS entries; each of the three may be NULL).  PJD_E_ARG if src_n or
 * dst_n is 0 or above 65535, i >= dst_n, or src_n > 16*dst_n.                                                                      */
#define PJD_RESIZE_BILINEAR  0
#define PJD_RESIZE_ANTIALIAS 1
#define PJD_AA_MAX_TAPS      32
int  pjd_batch_set_resize_filter(pjd_batch *b, int filter);
int  pjd_resize_aa_taps(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *first, uint32_t *count, uint32_t *q);   /* host only, no device needed */
/* ---- bicubic resize ---------------------------------------------------------------------------------------------------------- *
 * pjd_batch_set_resize_filter(b, PJD_RESIZE_BICUBIC): the resize of the batch uses Keys' cubic convolution kernel with a = -0.5,
 * WIDENED where an axis shrinks -- Pillow's BICUBIC (its bicubic_filter), torch.nn.functional.interpolate(mode="bicubic",
 * antialias=True) (_upsample_bicubic2d_aa), torchvision's Resize(InterpolationMode.BICUBIC, antialias=True): the filter timm's and
 * torchvision's ViT / DeiT / Swin / ConvNeXt / EfficientNet transforms use.  It is NOT the a = -0.75 kernel of torch's
 * NON-antialiased bicubic mode (interpolate(mode="bicubic", antialias=False), OpenCV's INTER_CUBIC), which differs visibly.
 *
 * THE ARITHMETIC (normative).  The source P is the source of pjd_batch_set_resize: the picture at its decode size, after
 * PJD_F_SCALE_*, with grey after an entropy-coding error.  Each axis is handled on its own.  Per axis, with sn source samples, dn
 * target samples, the target index i, S = max(sn, dn), T = 2*S and, for source sample j, D = |(2*j + 1)*dn - (2*i + 1)*sn| (exact
 * integers; D/T is the distance from the half-pixel centre in units of the support's scale):
 *     r_j =  3*D^3 - 5*T*D^2 + 2*T^3                    for D < T
 *     r_j =   -D^3 + 5*T*D^2 - 8*T^2*D + 4*T^3          for T <= D < 2*T          (zero or negative: the kernel's side lobe)
 * which is 2*T^3 * k(D/T), k(x) = 1.5|x|^3 - 2.5|x|^2 + 1 for |x| < 1 and -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 for 1 <= |x| < 2: support 2
 * target samples where the axis grows or stays, 2*sn/dn source samples where it shrinks.  Samples outside the picture are dropped
 * and the rest renormalised, as Pillow and torch do.  The TAPS are the contiguous run of j in 0..sn-1 with D < 2*T: `first` and
 * `count` are defined by the SUPPORT, not by r_j != 0 -- r_j is exactly 0 at D == T, which is inside the run: where sn == dn the taps
 * of an inner sample are (0, 65536, 0), and a target equal to the source size reproduces P byte for byte.  R = sum r_j > 0 always
 * (the centre lies inside the picture).  Quantised to 1/65536, SIGNED, divisions rounding DOWN (floor: round half up for either sign):
 *     q_j = floor((2*65536*r_j + R) / (2*R))
 * and then 65536 - sum q_j is added to the tap with the largest r_j (the lowest j on a tie), so that sum q_j == 65536 exactly.
 * r_j * 2^17 needs 69 bits at 65535-sample axes: the tap function uses 128-bit integers and is host only; the kernel divides
 * nothing.  Per channel, with (first, count, qx) of the target column and (first, count, qy) of the target row, all SIGNED 32-bit:
 *     h   = sum_x qx * P[y][x]                   (may be negative)
 *     h6  = (h + 512) >> 10                      (arithmetic shift: the row sample with 6 fraction bits)
 *     v   = sum_y qy * h6
 *     out = clamp((v + (1 << 21)) >> 22, 0, 255) (arithmetic shift)
 * One rounding of the intermediate, one final rounding, ONE clamp -- none between the passes: an overshoot of the horizontal pass
 * is carried into the vertical one, as the separable filter on float tensors carries it.  A constant picture stays constant.
 * RANGE.  With A = the largest sum |q_j| over the target samples of both axes, |h| <= 255*A, |h6| <= 255*A/1024 + 1 and
 * |v| <= A*|h6|: for A <= PJD_BICUBIC_MAX_GAIN = 92681 that is |h| <= 23 633 655, |h6| <= 23 080 and |v| + 2^21 <= 2 141 174 632
 * < 2^31, so every accumulator fits a signed 32-bit word, and every product has operands within 24 signed bits (|q| <= A < 2^17,
 * |h6| < 2^15, samples 8 bits).  The largest A found is 83 152 (gain 1.2688, the axis 14 -> 13 at i = 6: exhaustive over all admitted
 * axes below 130 samples, 200 000 sampled axes up to 65535; tests/test_resize_bicubic_cpu.py repeats the search), but the kernel
 * does not rest on that: pjd_batch_set_resize_filter sums |q_j| for every target sample of every table it builds and refuses an
 * axis above 92681 with PJD_E_ARG (pjd_last_error names the picture).
 * ERROR BOUND.  As for the triangle filter: a rounded q_j is within 1/2 of its exact value and the correction moves one tap by at
 * most n/2, so the absolute errors of an axis' n weights sum to at most n/65536: 255*n/65536 levels per axis, 0.2491 at the n = 64
 * of the limit below.  The horizontal error passes through the vertical pass with weights whose magnitudes sum to the gain
 * g <= 1.4142 (= 92681/65536; 1.2688 found): 0.2491*g; h6 adds its rounding, 1/128 level, times g; the vertical weights add their
 * own 0.2491 on samples that may overshoot to 255*g, i.e. 0.2491*g: at most (2*0.2491 + 1/128)*1.4142 = 0.716 levels (0.643 at the
 * gain found) from the exact separable filter before the ONE final rounding -- below 1, so the result is within 1 level of that
 * filter computed in float64, clamped once at the end and rounded to nearest, which is what torch computes on float tensors
 * (measured: 0.012 levels before rounding on random and 0/255 pictures, tests/test_resize_bicubic_cpu.py).
 * PILLOW'S uint8 PATH rounds and CLIPS the horizontal pass to 8 bits.  Where that pass overshoots 0..255 Pillow's result therefore
 * differs from the float64 filter, and from this one: by at most 1 level on smooth content, by up to 29 levels on a random 0/255
 * picture (measured, the same test).  That is a property of Pillow's 8-bit intermediate, not of the filter; it is not reproduced.
 * LIMIT.  sn <= 16*dn on each axis, as for the triangle filter.  PJD_BICUBIC_MAX_TAPS is the largest tap count the limit admits:
 * the points (2*j + 1)*dn inside an OPEN interval of length 4*T = 8*S, 2*dn apart: at most ceil(4*S/dn) -- 4 where the axis grows,
 * 64 where sn <= 16*dn, attained where the axis shrinks by exactly 16x, e.g. by 96 -> 6 at i = 3 (tests/test_resize_bicubic_cpu.py).
 *
 * CALL ORDER, the errors and everything "FROM THEN ON" are those of PJD_RESIZE_ANTIALIAS above, word for word: the 16x refusal that
 * names the picture, the window's limit and the tables of the windowed axes where the batch has source windows (their taps are
 * pjd_resize_bicubic_taps(w, vw, ox + i') and (h, vh, oy + j), addressed from x and y on), the weight table shared per (sn, dn)
 * pair and counted in device_bytes, the one launch named "resize", pjd_batch_set_normalize applied to `out`.
 * pjd_resize_bicubic_taps is the tap computation on its own, host only (no device needed), the very inline the table is built
 * with: first, count and q[0 .. count-1] (q has room for PJD_BICUBIC_MAX_TAPS entries; each of the three may be NULL).  PJD_E_ARG
 * if src_n or dst_n is 0 or above 65535, i >= dst_n, or src_n > 16*dst_n.                                                        */
#define PJD_RESIZE_BICUBIC      3   /* 2 is not a filter: it stays the unknown value callers were promised PJD_E_ARG for */
#define PJD_BICUBIC_MAX_TAPS    64
#define PJD_BICUBIC_MAX_GAIN    92681
int  pjd_resize_bicubic_taps(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *first, uint32_t *count, int32_t *q);   /* host only, no device needed */
/* ---- source windows: crop and flip inside the resize ------------------------------------------------------------------------------ *
 * pjd_batch_set_resize_window: picture i of a resized batch is resampled from a WINDOW of the decoded picture, to a window of a
 * VIRTUAL target, and mirrored left-right where asked (win: n_images records).  The pipelines of a vision loader in one launch:
 * RandomResizedCrop (x, y, w, h = the crop; vw, vh = 0), Resize(s) + CenterCrop(t) (the whole picture; vw x vh = the resized
 * size; ox, oy = where the centre crop starts), RandomHorizontalFlip (PJD_RW_HFLIP).  Every picture is still decoded whole: the
 * window lives in the resample launch alone.
 *
 * THE ARITHMETIC (normative).  P is the source of pjd_batch_set_resize: the sw x sh picture at its decode size, after
 * PJD_F_SCALE_*, with grey after an entropy-coding error; tw x th is the picture's target from pjd_batch_set_resize.  With the
 * defaults resolved (w == h == 0: x = y = 0, w = sw, h = sh; vw == 0: vw = tw; vh == 0: vh = th), for target column i and row j:
 *     i' = tw - 1 - i  with PJD_RW_HFLIP, else i
 *   bilinear:    (i0, i1, wx)     = pjd_resize_tap(w, vw, ox + i');      the source columns are x + i0 and x + i1
 *                (j0, j1, wy)     = pjd_resize_tap(h, vh, oy + j);       the source rows    are y + j0 and y + j1
 *                the blend and its ONE rounding are those of pjd_batch_set_resize
 *   antialiased: (first, count, q) = pjd_resize_aa_taps(w, vw, ox + i'); the source columns are x + first + t, t < count
 *                (first, count, q) = pjd_resize_aa_taps(h, vh, oy + j);  the source rows    are y + first + t
 *                h, h16, v and out are those of pjd_batch_set_resize_filter
 * The delivered picture is therefore flip(resize(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]): no new arithmetic, the two tap
 * functions above with a shifted index.  Samples outside the WINDOW are treated exactly as samples outside the picture are without
 * one -- clamped (bilinear), dropped and the rest renormalised (antialiased) -- and never contribute, even where the picture has
 * pixels there.  The error bounds of both filters carry over word for word.  An all-zero record is the identity; a batch whose
 * records are all zero delivers byte for byte what it delivers without the call.
 *
 * VALIDATION.  pjd_resize_window_check (host only, no device needed) is the one implementation; pjd_batch_set_resize_window calls
 * it for every picture with PJD_RESIZE_BILINEAR, pjd_batch_set_resize_filter again with the filter it is given.  PJD_OK, or
 * PJD_E_ARG (pjd_last_error names the picture) for: sw, sh, tw or th outside 1..65535, a null record, an unknown filter;
 * w == 0 xor h == 0; w == h == 0 with x or y non-zero; x + w > sw or y + h > sh; vw or vh above 65535; ox + tw > vw or
 * oy + th > vh (defaults resolved); an unknown flag bit; reserved_ != 0; and with PJD_RESIZE_ANTIALIAS or PJD_RESIZE_BICUBIC w > 16*vw
 * or h > 16*vh.
 * The 16x limit of the antialiased filter is the WINDOW's: a picture past 16x its target whose window is inside is accepted.
 *
 * CALL ORDER.  After pjd_batch_set_resize (and pjd_batch_set_orientation, below, where used); before any pjd_batch_set_resize_filter /
 * _set_normalize / _bind_output / _upload / _capture / _decode of the batch; once: PJD_E_STATE otherwise (so a batch that took pjd_batch_set_normalize without a resize
 * takes no window).  PJD_E_ARG for a null array or a record the check refuses; the batch is then as it was, un-windowed.
 * FROM THEN ON everything pjd_batch_set_resize promises from its "FROM THEN ON" holds unchanged -- sizes and offsets (those of
 * tw x th), every byte of every range written and none outside, the one launch named "resize", part of a captured graph, run again
 * after the exact-kernel fallback, bind_output and its alignment rules -- and pjd_batch_set_resize_filter and _set_normalize compose
 * as before: the weight table of the antialiased filter is built from the windowed axes (w, vw) and (h, vh).  The records (40 bytes
 * a picture) are counted in pjd_batch_info::device_bytes and sent by pjd_batch_upload; a batch whose records are all zero takes
 * none and runs the launch it ran before.  Status words, partial pictures, coefficients and pjd_plan_info are unaffected.      */
#define PJD_RW_HFLIP 1u
typedef struct pjd_resize_window {
    uint32_t x, y, w, h;   /* source window in P; w == h == 0 (then x == y == 0): the whole picture          */
    uint32_t vw, vh;       /* virtual target the window is resampled to; 0: the picture's target (tw / th)  */
    uint32_t ox, oy;       /* delivered: columns [ox, ox+tw), rows [oy, oy+th) of the virtual target        */
    uint32_t flags;        /* PJD_RW_HFLIP: the delivered picture mirrored left-right                       */
    uint32_t reserved_;    /* 0 */
} pjd_resize_window;
int  pjd_batch_set_resize_window(pjd_batch *b, const pjd_resize_window *win /* n_images */);
int  pjd_resize_window_check(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th,
                             const pjd_resize_window *win, int filter);   /* host only, no device needed */
/* ---- orientation: mirrors, half turn and quarter turns inside the resize ------------------------------------------------------------ *
 * pjd_batch_set_orientation: picture i of a resized batch is delivered in EXIF orientation orientation[i], 1..8 (tag 0x0112; what
 * pjd_scanned_orientation of pjd_host.h reads from the file, or any value the caller chooses: RandomVerticalFlip is 4, the quarter
 * turns of an augmentation 6 and 8).  The permutation happens in the resample launch, on the way out: no oriented copy exists.
 *
 * THE ARITHMETIC (normative).  out_w[i] x out_h[i] is picture i's target from pjd_batch_set_resize; that is what is DELIVERED, and
 * sizes and offsets never change.  The orientation o has the bits (t, v, h):
 *     o                      1  2  3  4  5  6  7  8
 *     t (transpose)          0  0  0  0  1  1  1  1
 *     v (mirror top-bottom)  0  0  1  1  0  0  1  1
 *     h (mirror left-right)  0  1  1  0  0  1  1  0
 * Q is the picture the batch would deliver with everything else it has -- window, virtual target, PJD_RW_HFLIP, filter -- to the
 * target out_w x out_h where t = 0 and to out_h x out_w, the axes swapped, where t = 1.  The delivered picture is
 *     D = H^h(V^v(T^t(Q)))        transpose first, then the mirrors
 * so o = 6 is Q turned a quarter clockwise (numpy.rot90(Q, -1)), o = 8 a quarter counter-clockwise (numpy.rot90(Q, 1)), o = 3 the half
 * turn; the table is PIL.ImageOps.exif_transpose's for all eight values.  pjd_batch_set_normalize applies to D's samples as it does to
 * Q's.  No new filter arithmetic: the resample happens in the STORED picture's coordinates and its result is permuted.  That differs
 * from "orient the picture, then resize it" only where a filter's tie-breaking is not mirror-symmetric -- the round-half-up of the
 * bilinear weight, the correction that goes to the lowest of equal taps -- and stays inside each filter's stated one-level bound,
 * as PJD_RW_HFLIP does.  A caller who wants the upright picture at its own size passes pjd_batch_set_resize the picture's own
 * dimensions, swapped for o >= 5: every tap weight is then 0 or 65536, and D is the exact permutation of the decoded picture.
 *
 * CALL ORDER.  After pjd_batch_set_resize; before any pjd_batch_set_resize_window / _set_resize_filter / _set_normalize /
 * _bind_output / _upload / _capture / _decode of the batch; once: PJD_E_STATE otherwise, also when no resize is set.  PJD_E_ARG for a
 * null array or a value outside 1..8 (pjd_last_error names the picture); the batch is then as it was.
 * FROM THEN ON, for a picture with t = 1, everything later calls say about "the target" is about Q's target out_h x out_w: the
 * defaults vw = 0 / vh = 0 of a window, ox + tw <= vw and oy + th <= vh, the 16x limit, the weight tables of (w, vw) and (h, vh).  A
 * window is given in the stored picture's coordinates, as without an orientation, and its PJD_RW_HFLIP mirrors Q.  Everything
 * pjd_batch_set_resize promises from its "FROM THEN ON" holds unchanged: pjd_batch_output_size, _offset, _packed_size, bind_output
 * and its alignment rules, both downloads; every byte of every range written by every decode and none outside; the one launch
 * named "resize", part of a captured graph, run again after the exact-kernel fallback.  What the call takes (the 40-byte record of
 * a window per picture) is counted in pjd_batch_info::device_bytes and sent by pjd_batch_upload; an array of all 1 takes nothing
 * and launches the very kernels the batch launched before.  A BMP batch takes no resize, so it takes no orientation.           */
int  pjd_batch_set_orientation(pjd_batch *b, const uint8_t *orientation /* n_images, each 1..8 */);
/* ---- pad on decode: the picture as a rectangle of a fixed canvas (letterbox) -------------------------------------------------------- *
 * pjd_batch_set_resize_pad: picture i of a resized batch fills only a rectangle of its target, and the rest of the target is set to a
 * fill colour -- keep the aspect ratio, pad what is left -- inside the resample launch and one small launch behind it: no padded copy
 * and no unpadded picture ever exists.
 *
 * THE CANVAS (normative).  out_w[i] x out_h[i] from pjd_batch_set_resize stays what is DELIVERED: the canvas.  Sizes, offsets,
 * pjd_batch_output_size, _packed_size, bind_output and both downloads never change.
 * THE CONTENT RECTANGLE of a record {left, top, right, bottom} is columns [left, out_w - right) and rows [top, out_h - bottom) of the
 * canvas: cw = out_w - left - right by ch = out_h - top - bottom samples, each at least 1.
 * THE TARGET.  From this call on, everything later calls say about "the target tw x th" is about cw x ch: for
 * pjd_batch_set_orientation and the orientations 5..8 Q's target is ch x cw; the defaults vw = 0 and vh = 0 of a window; the rules
 * ox + tw <= vw and oy + th <= vh; the 16x limit; the weight tables.
 * THE DELIVERED CANVAS.  Let D be the cw x ch picture the batch would deliver to a target of that size with everything else it has --
 * orientation, window, PJD_RW_HFLIP, filter.  Then
 *     C[c][y][x] = D[c][y - top][x - left]      for left <= x < out_w - right and top <= y < out_h - bottom
 *     C[c][y][x] = fill[c]                      everywhere else
 * No new filter arithmetic.  The pad is given in the DELIVERED canvas's coordinates: neither an orientation nor PJD_RW_HFLIP moves
 * or mirrors the rectangle; they act on D.
 * THE FILL.  pjd_batch_set_normalize applies to C's samples, the fill included: a border element of channel c is
 * pjd_normalize_value(dtype, fill[c], scale[c], bias[c]).  pjd_batch_set_pad_value replaces that for a normalised batch: a border
 * element of channel c is then value[c] converted ONCE to the dtype, to nearest even (the conversions of pjd_batch_set_normalize, no
 * fma) -- "zeros after normalisation" is value = {0, 0, 0}.
 *
 * CALL ORDER of pjd_batch_set_resize_pad.  After pjd_batch_set_resize; before any pjd_batch_set_orientation / _set_resize_window /
 * _set_resize_filter / _set_normalize / _bind_output / _upload / _capture / _decode of the batch; once: PJD_E_STATE otherwise, also when
 * no resize is set (a batch that took pjd_batch_set_normalize without a resize therefore takes no pad).  PJD_E_ARG for a null array, a
 * null fill, or a record with left + right >= out_w or top + bottom >= out_h (the sums in 64 bits; pjd_last_error names the picture);
 * the batch is then as it was and the call still open.  pjd_resize_pad_check is THE implementation of that test.
 * CALL ORDER of pjd_batch_set_pad_value.  After pjd_batch_set_normalize on a batch that took pjd_batch_set_resize_pad; before
 * _bind_output / _upload / _capture / _decode; once: PJD_E_STATE otherwise.  PJD_E_ARG for a null array or a value that is not finite.
 * FROM THEN ON every decode writes every byte of every picture's range, border included, and no byte outside it: the content by the
 * launch named "resize", the border by one named "pad" behind it, which write disjoint bytes; both are part of a captured graph and
 * run again after the exact-kernel fallback of pjd_batch_sync.  Status words, partial pictures (grey in the content, fill in the
 * border), coefficients and pjd_plan_info are unaffected; out_bytes stays the sum of the canvases.  What the call takes (a 32-byte
 * record and a 40-byte window per picture, one prefix sum) is counted in pjd_batch_info::device_bytes and sent by pjd_batch_upload.  An
 * array of all-zero records takes nothing: the batch launches the very kernels it launched before and delivers, byte for byte, what
 * it delivers without the call.  A BMP batch takes no resize, so it takes no pad.
 * VERSIONING.  No struct of this header changed, so PJD_VERSION stays 6; a caller checks for the feature by the symbol
 * pjd_resize_pad_check.                                                                                                          */
typedef struct pjd_resize_pad { uint32_t left, top, right, bottom; } pjd_resize_pad;
int  pjd_batch_set_resize_pad(pjd_batch *b, const pjd_resize_pad *pad /* n_images */, const uint8_t fill[3]);
int  pjd_batch_set_pad_value(pjd_batch *b, const float value[3]);
int  pjd_resize_pad_check(uint32_t out_w, uint32_t out_h, const pjd_resize_pad *pad);   /* host only, no device needed */
/* ---- affine warp on decode: rotate, scale, shear and translate per output ------------------------------------------------------------ *
 * pjd_batch_set_resize_affine: output i of a resized batch -- picture i, or view i after pjd_batch_set_views -- with target tw x th from
 * pjd_batch_set_resize is read from its picture under six doubles m[i] = {m00, m01, m02, m10, m11, m12}: the INVERSE map, from target
 * pixel centres to source pixel centres.  The one transform of a loader that is not separable -- every other setter of the resample is
 * a per-axis tap computation -- and so a launch of its own, which writes the fill where the target looks outside the picture too.
 *
 * THE ARITHMETIC (normative).  P is the sw x sh source of pjd_batch_set_resize: the picture at its decode size, after PJD_F_SCALE_* /
 * PJD_F_LIBJPEG_SCALE_*, grey behind an entropy-coding error.
 * SOURCE POSITION.  Target pixel (i, j) -- column i, row j -- looks at u = m00 * (i + 1/2) + m01 * (j + 1/2) + m02 and
 * v = m10 * (i + 1/2) + m11 * (j + 1/2) + m12; the centre of source pixel (x, y) is (x + 1/2, y + 1/2).
 * FIXED POINT, Q40.  Each coefficient is a = llrint(m * 2^40): an IEEE double product with a power of two (exact), rounded to nearest
 * even.  All further arithmetic is 64-bit two's-complement integer:
 *     X  = a00 * (2i + 1) + a01 * (2j + 1) + 2 * a02 - 2^40       2 * (u - 1/2) in Q40
 *     fx = (X + 2^32) >> 33                                      an arithmetic shift: u - 1/2 in 1/256 pixel, rounded to nearest
 *     x0 = fx >> 8  (the floor: may be negative)        wx = fx & 255
 * and Y, fy, y0, wy likewise from row 1 of the matrix.
 * TAPS.  The four taps are (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).  A tap with 0 <= x < sw and 0 <= y < sh reads
 * P[c][y][x], any other tap reads fill[c].  The blend and its one rounding are those of pjd_batch_set_resize:
 *     out = ((256 - wy) * ((256 - wx) * s00 + wx * s01) + wy * ((256 - wx) * s10 + wx * s11) + 32768) >> 16
 * every product with operands within 24 bits.  This is grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False) with
 * torchvision's mask blend towards `fill`.
 * LIMITS, checked on the quantised values: |a00|, |a01|, |a10|, |a11| <= 16 * 2^40 and |a02|, |a12| <= 2^18 * 2^40.  16 source pixels per
 * target pixel is the 16x of the table-driven filters.  Why nothing wraps: i, j <= 65534, so 2i + 1 < 2^17 and
 *     |X| <= 2^44 * 2^17 + 2^44 * 2^17 + 2 * 2^58 + 2^40 = 2^62 + 2^59 + 2^40 < 2^62.17,    |X + 2^32| < 2^62.3 < 2^63
 * and |fx| < 2^29.3: from fx on 32 bits hold everything.
 * CONSEQUENCES.  The identity matrix {1,0,0, 0,1,0} with tw = sw, th = sh reproduces P byte for byte: X = 2^40 * 2i, fx = 256 * i,
 * every weight is 0, and a tap outside with weight 0 contributes nothing.  Integer translations, mirrors and quarter turns are exact
 * permutations with `fill` where nothing maps: {0,-1,sw, 1,0,0} onto sh x sw is the quarter turn D[j][i] = P[i][sw - 1 - j].  A constant
 * picture under a map that stays inside stays constant (the weights of a blend sum to 65536).
 * ERROR BOUND.  Rounding fx is off by at most 1/512 pixel per axis.  Quantising the coefficients moves u by at most
 * 2^-41 * (i + 1/2) + 2^-41 * (j + 1/2) + 2^-41 < 2^-41 * 2^17 + 2^-41 < 2^-23 pixel.  A bilinear sample changes by at most 255 levels
 * per pixel of position on each axis, so the exact blend of the rounded position is within 255 * 2 * (1/512 + 2^-23) < 0.9963 levels
 * of the blend at the exact position, before the one rounding: the result is within 1 level of the same filter in float64 rounded
 * to nearest.
 * ALIASING.  Plain bilinear aliases where the map shrinks by more than about 2x: as with pjd_batch_set_resize, pre-scale with
 * PJD_F_SCALE_* and multiply the scale into the matrix.
 *
 * CALL ORDER.  After pjd_batch_set_resize, and after pjd_batch_set_views where used; before any pjd_batch_set_normalize / _bind_output /
 * _upload / _capture / _decode; once: PJD_E_STATE otherwise, also when no resize is set.  It is an ALTERNATIVE to the per-axis request,
 * not a layer on it: PJD_E_STATE on a batch that took pjd_batch_set_resize_pad, _set_orientation, _set_resize_window or
 * _set_resize_filter, and those four return PJD_E_STATE on a batch that took this call -- each of them is a matrix the caller
 * multiplies in.  PJD_E_ARG for a null array, a null fill, or a matrix pjd_resize_affine_check refuses (pjd_last_error names the
 * picture, or "view <v> (picture <p>)"); the batch is then as it was and the call still open.
 * COMPOSES WITH pjd_batch_set_normalize (fill is a sample like any other and goes through the fma: there is no pad value),
 * pjd_batch_bind_output, views (one matrix per view), PJD_OUT_RGB8, PJD_OUT_RGB8_PLANAR and PJD_OUT_GRAY8 (grey reads fill[0]),
 * PJD_F_LIBJPEG pictures, captured graphs, and the exact-kernel fallback of pjd_batch_sync, behind which the launch runs again.
 * FROM THEN ON everything pjd_batch_set_resize promises holds.  Every decode writes every byte of every output's range and none outside,
 * in ONE launch -- there is no border launch -- which pjd_batch_decode_timed names "warp".  The 48-byte record per output is counted in
 * pjd_batch_info::device_bytes and sent by pjd_batch_upload.  A batch that never makes the call allocates, uploads and launches what
 * it did before.
 * pjd_warp_tap and pjd_resize_affine_check are host only and THE implementations: the inline the kernel runs, and the test the setter
 * makes.  Both return PJD_E_ARG for a null matrix, a value that is not finite, a coefficient beyond the limits or a dimension outside
 * 1..65535; pjd_warp_tap also for i or j at or above 65535.  Its outputs may be NULL.
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for the symbol pjd_warp_tap.                              */
int  pjd_batch_set_resize_affine(pjd_batch *b, const double (*m)[6] /* n outputs */, const uint8_t fill[3]);
int  pjd_warp_tap(const double m[6], uint32_t i, uint32_t j, int64_t *x0, int64_t *y0, uint32_t *wx, uint32_t *wy);   /* host only */
int  pjd_resize_affine_check(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const double m[6]);                /* host only */
/* ---- colour map on decode: a 3 x 4 colour map per output ------------------------------------------------------------------------------ *
 * pjd_batch_set_colour: output i of a resized batch -- picture i, or view i after pjd_batch_set_views -- has its resampled 8-bit triple
 * (R, G, B) replaced by m[i] applied to it, twelve doubles, row-major: out[c] = m[4c] * R + m[4c+1] * G + m[4c+2] * B + m[4c+3], the last
 * column in 8-bit levels.  Inside the one resample or warp launch, before the normalisation and the store: brightness, contrast about a
 * constant, saturation, hue, grey, channel order and any product of them are one such matrix.
 *
 * THE ARITHMETIC (normative).  R, G, B are the samples the resample delivers: the 8-bit values that would be stored without this call,
 * whatever filter, window, orientation or affine map made them.
 * FIXED POINT, Q16.  q[c][k] = llrint(m[4c+k] * 65536) for k = 0..2 and o[c] = llrint(m[4c+3] * 65536): an IEEE double product with a power
 * of two (exact), rounded to nearest even.  Then
 *     out[c] = clamp((q[c][0] * R + q[c][1] * G + q[c][2] * B + o[c] + 32768) >> 16, 0, 255)
 * Everything is 32-bit signed two's complement, the shift is arithmetic, and there is ONE clamp, at the end.
 * LIMITS, checked on the quantised values: |q| <= 2^20 (|weight| <= 16) and |o| <= 2^28 (|offset| <= 4096 levels); every value finite.  No sum
 * can wrap: 3 * 255 * 2^20 + 2^28 + 2^15 = 1 070 628 864 < 2^31.  Every product has operands of at most 24 signed bits (v_mad_i32_i24).
 * CONSEQUENCES.  The identity, the six channel permutations, any 0/1 selection matrix and integer offsets are exact: q * v is a multiple
 * of 65536, the rounding term shifts out.  Against the same map in float64, with x = m[4c] * R + m[4c+1] * G + m[4c+2] * B + m[4c+3]
 * unrounded, |out - clamp(x, 0, 255)| <= 0.5 + 2^-7: the one rounding is half a level, and quantising the weights contributes at most
 * (3 * 255 + 1) * 2^-17 = 0.00585 levels.
 * ORDER.  The normalisation of pjd_batch_set_normalize reads out[c].  Under pjd_batch_set_resize_affine the fill takes part in the blend as
 * any sample does, so it passes through the map (torchvision's order: RandomAffine before ColorJitter).  Under pjd_batch_set_resize_pad
 * the border is not content: it stays the fill / the pad value as given, and the border launch is unchanged.
 *
 * CALL ORDER.  After pjd_batch_set_resize and whatever shapes the resample (pad, orientation, window, filter, affine map; after
 * pjd_batch_set_views where used: one matrix per OUTPUT); before pjd_batch_set_normalize / _bind_output / _upload; once: PJD_E_STATE
 * otherwise, also when no resize is set.  PJD_E_ARG for a PJD_OUT_GRAY8 batch (one plane has no colour map: gain and offset are the
 * normalisation's), a null pointer, or a matrix pjd_colour_check refuses (pjd_last_error names the picture, or "view <v> (picture <p>)");
 * the batch is then as it was and the call still open.
 * COMPOSES WITH all three filters, windows, orientations, pad, views, the affine warp, pjd_batch_set_normalize (all element types),
 * PJD_OUT_RGB8 and PJD_OUT_RGB8_PLANAR, pjd_batch_bind_output, PJD_F_LIBJPEG pictures, both scale families, captured graphs, and the
 * exact-kernel fallback of pjd_batch_sync, behind which the launch runs again.
 * FROM THEN ON everything pjd_batch_set_resize promises holds; pjd_batch_decode_timed keeps the names "resize", "pad" and "warp".  The
 * 64-byte record per output is counted in pjd_batch_info::device_bytes and sent by pjd_batch_upload.  A map that is the identity after
 * quantisation is skipped by the kernel (the same bytes: the identity is exact).  A batch that never makes the call allocates, uploads
 * and launches what it did before.
 * pjd_colour_value and pjd_colour_check are host only and THE implementations: the inline the kernels run, and the test the setter
 * makes.  pjd_colour_value returns PJD_E_ARG for a null pointer or a matrix beyond the limits; pjd_colour_check returns 1 for a matrix the
 * setter accepts and 0 for one it refuses (null included).
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for the symbol pjd_colour_value.                         */
int  pjd_batch_set_colour(pjd_batch *b, const double (*m)[12] /* pjd_batch_n_outputs(b) */);
int  pjd_colour_value(const double m[12], const uint8_t rgb[3], uint8_t out[3]);   /* host only, no device needed */
int  pjd_colour_check(const double m[12]);                                        /* host only: 1 ok, 0 refused */
/* ---- Gaussian blur on decode: a separable blur per output ----------------------------------------------------------------------------- *
 * pjd_batch_set_blur: output i of a resized batch -- picture i, or view i after pjd_batch_set_views -- leaves as the separable Gaussian of
 * what the batch would deliver without the call, in one more launch behind the resample (or the warp): torchvision's GaussianBlur of the
 * SimCLR, MoCo v2, BYOL, DINO and SwAV recipes, between the colour ops and the normalisation.
 *
 * MEANING (normative).  Let U be the uint8 output the same batch delivers without this call and without pjd_batch_set_normalize: after
 * whatever filter, window, orientation, views, affine warp (fill included) and colour map are set, and whatever PJD_F_* made the picture.
 * An output with ksize == 0 (sigma must then be 0) is U, byte for byte.  Otherwise the output is the separable Gaussian of U over the whole
 * tw x th output, the same taps on both axes, each channel on its own.
 * TAPS.  ksize is odd and within 1..PJD_BLUR_MAX_TAPS, r = ksize / 2; sigma is finite and greater than 0.  In IEEE double:
 *     w[j] = exp(-0.5 * ((j - r) / sigma)^2),  t = w[0] + w[1] + ... in index order,  q[j] = llrint(w[j] / t * 65536),
 * then q[r] += 65536 - sum(q).  The taps are symmetric, non-negative and sum to exactly 65536 (the centre is the largest tap, of at least
 * 65536 / ksize, and the correction at most ksize / 2 in magnitude).  The HOST builds the table once per distinct (ksize, sigma) of a batch
 * (pjd_blur_taps is that code); the kernel reads it and never evaluates exp.
 * BORDER.  torchvision's "reflect", defined for every size: sample i of an axis of n samples is sample idx(i), where for n == 1
 * idx(i) = 0 and otherwise, with p = 2 * (n - 1): m = i mod p (0 <= m < p), idx(i) = m < n ? m : p - m.  A halo wider than the output
 * folds several times.  pjd_blur_index is this rule.
 * ARITHMETIC.  Unsigned 32-bit, the triangle filter's own (pjd_batch_set_resize_filter, PJD_RESIZE_ANTIALIAS).  Horizontal first:
 *     h   = sum_j q[j] * U[y][idx(x + j - r)]             at most 255 * 65536 < 2^24
 *     h8  = (h + 128) >> 8                                 the row sample, at most 65280: 16 bits
 *     v   = sum_j q[j] * h8[idx(y + j - r)][x]             v + 2^23 is at most 65536 * 65280 + 2^23 = 4 286 578 688 < 2^32
 *     out = (v + 2^23) >> 24
 * CONSEQUENCES.  A table whose only non-zero tap is the centre (ksize 1; sigma 0.1 at any ksize) is the identity, exactly: h8 = 256 * U
 * and out = U; the kernel skips nothing but reads that one tap.  A constant picture stays constant, for the taps sum to 65536.  Against
 * the same filter in float64 (the unquantised w[j] / t, no intermediate rounding) the result differs by less than one level: half a level
 * for the final rounding, 2^-9 for the row sample (half a unit of h8, 1/256 level, through vertical taps that sum to 1), and per axis at
 * most ksize * 2^-16 * 255 for the taps -- each within 2^-17 of its value before the centre takes up to ksize * 2^-17 more -- so
 * 0.5 + 0.002 + 2 * 63 * 255 / 65536 = 0.993 at 63 taps (0.506 was the worst found by the model of tests/blur_model.py).  It is within one
 * level of torchvision.transforms.v2.functional.gaussian_blur on the uint8 tensor wherever r < min(tw, th), torch's own limit for reflect
 * padding.  Pillow's ImageFilter.GaussianBlur is a box approximation and is NOT reproduced.
 * ORDER.  The normalisation of pjd_batch_set_normalize reads the blurred byte.
 *
 * CALL ORDER.  After pjd_batch_set_resize and everything that shapes the resample, pjd_batch_set_colour included (after pjd_batch_set_views
 * where used: one entry per OUTPUT); before pjd_batch_set_normalize / _bind_output / _upload; once: PJD_E_STATE otherwise, also when no
 * resize is set, and for a shaping setter called behind it.  PJD_E_ARG for a null pointer, an entry pjd_blur_check refuses (an even ksize,
 * one above PJD_BLUR_MAX_TAPS, a sigma that is not finite or not positive with ksize > 0, a non-zero sigma with ksize == 0, a non-zero
 * reserved_; pjd_last_error names the picture, or "view <v> (picture <p>)"), and for a batch with pjd_batch_set_resize_pad: the border
 * there is not content, and a pad value has no 8-bit form.  The batch is then as it was and the call still open.
 * COMPOSES WITH all three filters, windows, orientations, views, the affine warp, the colour map, PJD_OUT_RGB8, PJD_OUT_RGB8_PLANAR and
 * PJD_OUT_GRAY8 (one channel), pjd_batch_set_normalize (all element types), pjd_batch_bind_output (any element-aligned offset),
 * PJD_F_LIBJPEG pictures, both scale families, captured graphs, and the exact-kernel fallback of pjd_batch_sync, behind which the launch
 * runs again.
 * HOW.  The resample (or warp) launch of a blurred batch writes U, uint8 and not normalised, into one more intermediate buffer of the
 * batch (the packed layout of the uint8 outputs); the blur launch reads it and writes the final ranges, normalised where asked for.
 * Outputs with ksize == 0 pass through that launch as a copy.  Every decode writes every byte of every output's range and none outside
 * it, and every byte of the intermediate buffer that the blur launch reads.  pjd_batch_decode_timed names the launch "blur", behind
 * "resize" or "warp".  The buffer, one 40-byte record per output, the tile prefix and the tap table are counted in
 * pjd_batch_info::device_bytes and sent by pjd_batch_upload.  A batch that never makes the call allocates, uploads and launches what it
 * did before.
 * pjd_blur_taps, pjd_blur_index and pjd_blur_check are host only and THE implementations.  pjd_blur_taps and pjd_blur_index return
 * PJD_E_ARG for a null pointer or arguments beyond the limits (n is 1..65535); pjd_blur_check returns 1 for an entry the setter accepts
 * and 0 for one it refuses (null included).
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for the symbol pjd_blur_taps.                               */
#define PJD_BLUR_MAX_TAPS 63
typedef struct pjd_blur { double sigma; uint32_t ksize; uint32_t reserved_; } pjd_blur;
int  pjd_batch_set_blur(pjd_batch *b, const pjd_blur *blur /* pjd_batch_n_outputs(b) */);
int  pjd_blur_taps(uint32_t ksize, double sigma, uint32_t *q /* ksize */);         /* host only */
int  pjd_blur_index(uint32_t n, int64_t i, uint32_t *src);                         /* host only: the border rule */
int  pjd_blur_check(const pjd_blur *blur);                                         /* host only: 1 ok, 0 refused */
/* ---- normalised float output ------------------------------------------------------------------------------------------------- *
 * pjd_batch_set_normalize: the pictures of the batch leave the decode as floating-point elements, sample * scale[c] + bias[c] -- what
 * x.float().div(255).sub(mean).div(std).to(dtype) makes of the uint8 tensor, without that tensor ever existing.  The caller passes
 * scale[c] = 1 / (255 * std[c]) and bias[c] = -mean[c] / std[c]; any finite values are allowed.
 *
 * THE ARITHMETIC (normative).  Let P' be the uint8 picture the batch would deliver without this call -- the reference's picture, or
 * the partial picture with grey after an entropy-coding error, after PJD_F_SCALE_* and after pjd_batch_set_resize if one is set.
 * Every sample v = P'[c][y][x] of channel c (0 = R, 1 = G, 2 = B) leaves as
 *     u   = fma((float)v, scale[c], bias[c])     one IEEE binary32 fused multiply-add: the exact value of v*scale + bias, rounded
 *                                                once, to nearest even
 *     out = u                                    PJD_DT_F32
 *         = u rounded to binary16, nearest even  PJD_DT_F16  (subnormals kept, overflow gives infinity)
 *         = u rounded to bfloat16, nearest even  PJD_DT_BF16 (bits = u's 32 bits; bits += 0x7fff + ((bits >> 16) & 1); out = bits >> 16)
 * Elements are stored little-endian.  The fused form is deliberate: the compiler contracts a multiply and an add into the fma
 * anyway, so it is written as one and does not depend on a build's contraction flags.  (An unfused float32 multiply-then-add gives
 * other binary32 results on about half of the 256 levels with the ImageNet constants: tests/test_normalize_cpu.py.)
 * pjd_normalize_value is that computation for one sample v <= 255, host only (no device needed); its fma stage is the very inline
 * the kernel runs.  It writes 2 or 4 bytes to `out`; PJD_E_ARG for a dtype other than the three, v > 255, a non-finite scale or
 * bias, a null `out`.
 *
 * CALL ORDER.  After pjd_batch_create, and after pjd_batch_set_resize if that is used; before any pjd_batch_bind_output / _upload /
 * _capture / _decode of the batch; once: PJD_E_STATE otherwise.  PJD_E_ARG for a null array, a dtype other than the three, a
 * non-finite scale or bias, a PJD_OUT_BMP batch, a batch that holds a shard (the exclusions of pjd_batch_set_resize).
 * WITHOUT A RESIZE the call acts as if pjd_batch_set_resize had been called with every picture's own output size: every tap weight
 * is then 0 and P' is the unresized picture byte for byte; the batch gains the intermediate buffer described there, and a later
 * pjd_batch_set_resize returns PJD_E_STATE.
 * FROM THEN ON an element has 2 (PJD_DT_F16, PJD_DT_BF16) or 4 (PJD_DT_F32) bytes: PJD_OUT_RGB8_PLANAR gives dtype[3][th][tw],
 * PJD_OUT_RGB8 dtype[th][tw][3]; pjd_batch_output_size(b, i) is 3 * tw * th * sizeof(dtype); pjd_batch_output_offset, _packed_size,
 * _device_output, _download and _download_packed move bytes as before; pjd_batch_bind_output, pjd_batch_info::out_bytes and
 * device_bytes follow the larger elements.  The library's own offsets stay 256-byte aligned; pjd_batch_bind_output requires
 * device_base + offsets[i] to be a multiple of the element size (PJD_E_ARG otherwise) and nothing beyond that.  Every decode writes
 * every byte of every picture's range and no byte outside it.  The work is still the one launch behind the back end
 * (pjd_batch_decode_timed still names it "resize"; part of a captured graph; it runs again after the exact-kernel fallback of
 * pjd_batch_sync).  Status words, coefficients and pjd_plan_info are unaffected.                                                  */
#define PJD_DT_F16   1   /* IEEE binary16 */
#define PJD_DT_BF16  2   /* bfloat16 */
#define PJD_DT_F32   3   /* IEEE binary32 */
int  pjd_batch_set_normalize(pjd_batch *b, int dtype, const float scale[3], const float bias[3]);
int  pjd_normalize_value(int dtype, uint32_t v, float scale, float bias, void *out);   /* host only, no device needed */
/* ---- views: several resampled outputs of one decoded picture --------------------------------------------------------------------- *
 * pjd_batch_set_views: the batch delivers n_views OUTPUTS instead of one per picture; view v is a resample of picture
 * picture_of_view[v] -- two augmented views of every picture (SimCLR, MoCo, BYOL), 2 global + 6..10 local crops (DINO, SwAV),
 * FiveCrop / TenCrop, one picture at two resolutions, one large picture cut into tiles.  Every picture is still decoded whole and
 * ONCE: the entropy decoder and the back end do the work of n_images pictures, the resample launch that of n_views outputs.
 *
 * MEANING (normative).  View v is an output of its own.  Its source P is the picture that picture_of_view[v] produces at its decode
 * size -- after PJD_F_SCALE_* / PJD_F_LIBJPEG_SCALE_*, with grey behind an entropy-coding error: exactly the P of pjd_batch_set_resize.
 * Views may name pictures in any order; a picture may have any number of views, zero included (it is still decoded and still has its
 * status word).  No new arithmetic: each view is what a one-view batch would deliver for that picture with the same setters.
 *
 * CALL ORDER.  After pjd_batch_create; before any pjd_batch_set_resize / _set_normalize / _bind_output / _upload / _capture / _decode
 * of the batch; once: PJD_E_STATE otherwise.  PJD_E_ARG for a null array, n_views == 0 or above PJD_MAX_VIEWS, an entry >= n_images
 * (pjd_last_error names the view), a PJD_OUT_BMP batch.  After a failure the batch is as it was and the call is still open.
 * PJD_MAX_VIEWS bounds the page-locked record arrays of a batch (about 130 bytes a view with every record kind in use: 8.5 MB at
 * the cap); it is a bound of this header, NOT a measured figure.
 * FROM THEN ON the output index is the VIEW.  Every per-picture array of the resample setters has n_views entries, indexed by view:
 * out_w / out_h of pjd_batch_set_resize, pad of pjd_batch_set_resize_pad, orientation of pjd_batch_set_orientation, win of
 * pjd_batch_set_resize_window.  So have offsets of pjd_batch_bind_output and out of pjd_batch_download; the index of
 * pjd_batch_output_size / _output_offset / _device_output is the view; pjd_batch_packed_size and pjd_batch_download_packed speak about
 * the packed views; pjd_batch_info::out_bytes is the sum over the views.  What stays per PICTURE: status of both downloads and
 * pjd_batch_device_status (n_images words), pjd_batch_download_coefficients, and n_images, pixels and every planning figure of
 * pjd_batch_info (n_subsequences, n_huff_workgroups, n_data_units, ...: those of the batch without views).
 * THE SETTERS.  Every rule, limit, call order and error of pjd_batch_set_resize, _set_resize_pad, _set_orientation,
 * _set_resize_window, _set_resize_filter, _set_normalize and _set_pad_value holds word for word PER VIEW, each view against its own
 * picture's decode size; where pjd_last_error names a picture it names the view: "view <v> (picture <p>): ...".  A view of a shard is
 * refused by pjd_batch_set_resize (and by pjd_batch_set_normalize), as a shard is without views.  pjd_batch_set_normalize without a
 * resize acts as if pjd_batch_set_resize had been called with each view's own picture's output size.
 * VIEWS NEED THE RESAMPLE: pjd_batch_bind_output, _upload, _capture and _decode return PJD_E_STATE on a batch that has views but
 * neither a resize nor a normalisation (until then pjd_batch_output_size / _offset answer with the view's picture's).
 * GUARANTEES.  Every decode writes every byte of every view's range and no byte outside it.  The work is still the one launch named
 * "resize", plus "pad" where there are borders; both are part of a captured graph and run again after the exact-kernel fallback of
 * pjd_batch_sync.  No kernel is new or changed: the resample's records (source offset and size, target, window, pad, tables) were
 * always self-contained, and two records may read one source.  IDENTITY: picture_of_view = {0, 1, .., n_images - 1} delivers byte for
 * byte what the batch delivers without the call, and launches the same kernels.
 * COST.  The records, one set per view, are counted in pjd_batch_info::device_bytes and sent by pjd_batch_upload; the intermediate
 * buffer is per picture, as without views.  One launch covers fewer than 2^31 tiles and 2^31 border lines, summed over the views
 * in 64 bits: a request beyond that is refused with PJD_E_ARG by the setter that reaches it, never wrapped.
 * OUT OF SCOPE: pjd_pipeline.h (the batcher's sink stays per picture), bin/decoder, pjd_split_decode, pjd_decode_batch.
 * DETECTION.  No struct changed and PJD_VERSION stays 6: a caller checks for the symbol pjd_batch_n_outputs -- n_views once views
 * are set, else n_images; 0 for NULL.                                                                                                */
#define PJD_MAX_VIEWS 65536u
int  pjd_batch_set_views(pjd_batch *b, const uint32_t *picture_of_view, uint32_t n_views);
uint32_t pjd_batch_n_outputs(pjd_batch *b);
int  pjd_batch_get_info(pjd_batch *b, pjd_batch_info *info);
uint64_t pjd_batch_output_size(pjd_batch *b, int image);
void *pjd_batch_device_output(pjd_batch *b, int image);      /* device pointer (HBM)          */
void *pjd_batch_device_status(pjd_batch *b);                 /* int32[n_images] in HBM        */
void pjd_batch_destroy(pjd_batch *b);

/* ---- stage-level parity (debug; not on the product path) ------------------------------------ *
 * The coefficients of one image as the entropy decoder left them, in the layout of the reference's
 * MCU_buffer after decode_Huffman_data (jpeg_scanner.cpp:733-741): n_dpus x int16[19200], index
 * blk16 * 768 + component * 256 + position * 64 + natural index (through the reference's zigzag_map,
 * common.h:9-18), absolute DC values, zero where nothing was decoded.  n_dpus x 19200 =
 * pjd_coefficients_size(...) as decoder_host.cpp:125-128 sizes it.  Works after pjd_batch_decode for
 * images of either path (lane streams / exact kernel); an image the parallel decoder handed to the
 * exact kernel is decoded once more for this call.  Synchronises the stream.                          */
uint64_t pjd_coefficients_size(uint32_t width, uint32_t height, uint8_t h_samp, uint8_t v_samp);   /* in int16 */
int  pjd_batch_download_coefficients(pjd_batch *b, int image, int16_t *out, uint64_t capacity_int16);

/* One call: create + upload + decode + download + destroy.                    */
int  pjd_decode_batch(pjd_ctx *ctx, const pjd_image_desc *images, int n_images,
                      int out_format, uint8_t *const *out, int32_t *status);

/* ---- one picture over several devices (BASELINE config 5) -------------------------------------- *
 * Replaces what the reference does with every picture -- spread it over all allocated DPUs, copy the metadata
 * to each and collect the samples (decoder_host.cpp:125-149,225,262-312) -- for a picture with restart
 * intervals: device k of `devices` decodes a contiguous range of restart segments (pjd_split_plan), the
 * descriptor (tables + segment offsets, ~20 KB) is broadcast from the first device's HBM with one
 * ncclBroadcast (RCCL over xGMI; loaded on first use; plain copies if RCCL is missing), every device
 * uploads only its slice of `desc->ecs`, and the rows come back into `out` (pjd_image_output_size bytes: at the output scale).
 * One host thread per device inside the call.  A picture that cannot be split (no DRI; subsampled luma
 * under the reference's restart rule) is decoded by devices[0] alone; so is, a second time, a picture whose
 * entropy decode reports an error, so that status and partial picture are the reference's.               */
#define PJD_SPLIT_MAX_DEVICES 16
typedef struct pjd_split_stats {
    double   wall_s, broadcast_s, upload_s, exec_s, download_s;   /* the three stages: slowest rank          */
    uint64_t blob_bytes;               /* size of the broadcast descriptor                                  */
    uint64_t ecs_bytes[PJD_SPLIT_MAX_DEVICES];   /* entropy-coded bytes each rank uploaded                  */
    uint32_t n_segments, n_ranks;      /* restart segments of the picture; ranks that had work              */
    uint32_t n_exact;                  /* shards the exact one-lane kernel decoded                          */
    int32_t  rccl_used;                /* 1: the descriptor travelled by ncclBroadcast                      */
    int32_t  redone_whole;             /* 1: decoded again on one device after an entropy-coding error      */
} pjd_split_stats;
int  pjd_split_decode(const pjd_image_desc *desc, const int32_t *devices, int n_devices, int out_format,
                      uint8_t *out, uint64_t capacity, int32_t *status, pjd_split_stats *stats);
/* The range arithmetic on its own (no device needed): rank `rank` of `world` takes segments
 * [shard_first_seg, +shard_n_segs) = bytes [*byte_lo, *byte_hi) of desc->ecs = MCUs [*first_mcu, *last_mcu).
 * `shard` (optional, with `seg_scratch`: desc->n_segments words that must outlive it) becomes the descriptor
 * that rank passes to pjd_batch_create: its ecs points at the slice, its offsets are relative to the slice.
 * Returns PJD_OK, 1 if the rank has no segment (more ranks than segments), PJD_E_ARG.                      */
int  pjd_split_plan(const pjd_image_desc *desc, int world, int rank, pjd_image_desc *shard, uint64_t *seg_scratch,
                    uint64_t *byte_lo, uint64_t *byte_hi, uint32_t *first_mcu, uint32_t *last_mcu);
void pjd_split_release(void);          /* drops the cached RCCL communicators                               */
/* Diagnostic: the RCCL leg of pjd_split_decode on ONE device -- librccl is loaded, a one-rank communicator created, `bytes` bytes of
 * a pattern broadcast (root 0) from one HBM buffer into another on the library's stream, the result compared, the communicator
 * destroyed.  Exercises exactly the calls pjd_split_decode makes (ncclCommInitAll / ncclGroupStart / ncclBroadcast / ncclGroupEnd /
 * ncclCommDestroy) on boxes that have a single GPU.  0: ok; PJD_E_STATE: librccl cannot be loaded; PJD_E_HIP: a call failed.          */
int  pjd_split_rccl_selftest(int device_ordinal, uint64_t bytes);

/* ---- the literal DPU contract ---------------------------------------------- *
 * metadata: n_dpus x u32[276]   (decoder_host.cpp:156-178 index map)
 * mcus    : n_dpus x i16[19200] coefficients in, R/G/B samples out, both in the
 *           reference's blk16 layout (decoder_dpu.c:134-156,361-390).
 * Replaces copy/copy/exec/copy of decoder_host.cpp:276-308 one for one.        */
int  pjd_exec_dpu_payload(pjd_ctx *ctx, const uint32_t *metadata, int16_t *mcus, int n_dpus);

/* Host-only planning: what a batch of these images would occupy (no device needed).
 * Fills everything in `info` except device_bytes / n_fallback.  Plans as a context
 * opened now would: PJD_PLAN_MODE and PJD_SUB_BYTES (a subsequence size forced for the
 * whole batch, a multiple of 64 in 128..1024) of the environment apply, as in pjd_open. */
int  pjd_plan_info(const pjd_image_desc *images, int n_images, int out_format, pjd_batch_info *info);
/* Host-only: would pjd_batch_create take these images?  Runs the planner's tests and returns its code; `text` (cap bytes, always
 * terminated; may be NULL) receives "" or the reason pjd_last_error would report after pjd_batch_create ("image <i>: ..." where one
 * picture is at fault).  What a caller that ORs one set of flags into many descriptors uses to sort out, picture by picture, the ones
 * a flag does not take (PJD_F_LIBJPEG on 4:4:0 sampling, for one) before it builds its batch.                                       */
int  pjd_plan_check(const pjd_image_desc *images, int n_images, int out_format, char *text, uint64_t cap);
/* Debug, host-only: the bound behind the size of a picture's lane streams -- the fewest bits of bitstream per step of the entropy
 * decoder's write pass (one symbol, or the pair one table lookup yields) that ANY stream coded with this picture's Huffman tables can
 * sustain, x 256 (the minimum mean weight of a cycle of the step graph, pim-jpeg-decoder_amd/csrc/pjd_plan.cpp).  PJD_E_ARG for a
 * picture that does not take the parallel decoder.  tests/test_planner_bound.py recomputes it another way.                        */
int  pjd_plan_step_bits(const pjd_image_desc *image, uint32_t *step_bits_x256);
/* Debug, host-only: the decode tables of a picture's table set as the entropy decoder holds them in LDS, built in host memory by the
 * text the device builds them with (pim-jpeg-decoder_amd/csrc/pjd_lut_build.h; the layout: pjd_internal.h, PjdDevTset).
 * *real_bytes: the size of the blob (a multiple of 16; 0: the set takes the exact kernel and has no decode tables).  *nominal_bytes: its
 * size at 256 bytes per 9-bit prefix that starts longer codes -- the figure that ROUTES a set (over 20,480: the exact kernel), which
 * the blob itself no longer reaches.  `slots` (6 bytes, may be NULL): [component][0 = DC, 1 = AC] -> which 2,048-byte first-level
 * table of the blob the component decodes with.  `blob` (may be NULL: the sizes alone) receives *real_bytes bytes; PJD_E_ARG where
 * `cap` is smaller, and for a progressive frame (no table set: the scans bring their tables).  tests/test_lut_layout.py checks
 * every 16-bit window of it against a canonical matcher.                                                                          */
int  pjd_plan_luts(const pjd_image_desc *image, void *blob, uint64_t cap, uint32_t *real_bytes, uint32_t *nominal_bytes, uint8_t *slots);
/* Debug: what the runtime answers for the entropy decoder's launch of this batch on its device
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor): workgroups of pjd_k_huff_lanes one CU holds at the batch's dynamic LDS, and that
 * size (`lds_bytes`, may be NULL: pjd_batch_info.huff_lds_bytes).  Also printed by
 * pjd_batch_get_info under PJD_DEBUG_STATS.                                                                                       */
int  pjd_batch_huff_occupancy(pjd_batch *batch, int32_t *workgroups_per_cu, uint32_t *lds_bytes);

/* Page-locked host memory (hipHostMalloc) for pjd_batch_download_packed; NULL on failure.       */
void *pjd_host_alloc(uint64_t bytes);
void pjd_host_free(void *p);

/* Size in bytes of one picture in a given output format.                      */
uint64_t pjd_output_size(uint32_t width, uint32_t height, int out_format);
/* Channels of an output format: 3 for PJD_OUT_RGB8, PJD_OUT_BMP and PJD_OUT_RGB8_PLANAR, 1 for PJD_OUT_GRAY8, 0 for a value that is
 * no format.  Host only (no device needed).  PJD_OUT_GRAY8 changed no struct and no version: a caller that needs it checks for it by
 * this symbol, which is exported from the first library that knows the format.                                                    */
int  pjd_output_channels(int out_format);
/* Output dimensions of a width x height picture under descriptor flags `flags` (PJD_F_SCALE_*, or PJD_F_LIBJPEG_SCALE_*): ceil(W/s) x ceil(H/s).  Returns PJD_OK. */
int  pjd_scaled_dims(uint32_t width, uint32_t height, uint32_t flags, uint32_t *out_w, uint32_t *out_h);
/* Size in bytes of the picture of one descriptor in a given output format, at its output scale: what pjd_batch_output_size,
 * pjd_decode_batch and pjd_split_decode use.  0 for a null descriptor.                                                       */
uint64_t pjd_image_output_size(const pjd_image_desc *d, int out_format);

#ifdef __cplusplus
}
#endif
#endif /* PJD_H */
