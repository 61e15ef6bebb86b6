// pjd_internal.h -- data layout shared by the host planner and the gfx950 kernels.
//
// Everything the kernels read lives in HBM in these plain structs / arrays; the
// host planner (pjd_plan.cpp) fills them from pjd_image_desc, the API
// (pjd_api.hip) uploads them once per batch.
#pragma once
#include <stdint.h>

// ---- tunables -----------------------------------------------------------------
#ifndef PJD_SUB_BYTES_MIN
#define PJD_SUB_BYTES_MIN  128      // Huffman subsequence (bytes of bitstream per decode lane): chosen per batch (a multiple of 64)
#endif                              //   and then per picture (a multiple of 16: PJD_WORD_ROWS a multiple of 4, checkpoints on word
#define PJD_SUB_BYTES_MAX  1024     //   boundaries) by the planner, in this range, see pjd_plan.cpp
#define PJD_HUFF_LANES     64       // subsequences per wave: lanes exchange states by shuffles, no barriers
#ifndef PJD_HUFF_WAVES
#define PJD_HUFF_WAVES     2        // waves per Huffman workgroup; they share one table set in LDS
#endif
#define PJD_HUFF_THREADS   (PJD_HUFF_LANES * PJD_HUFF_WAVES)
#ifndef PJD_NCHK
#define PJD_NCHK           4        // checkpoints per subsequence (trajectory states a re-sync bridge can merge into); a power of two
#endif
#define PJD_STAGE_ENTRIES  16       // slots a lane stages in LDS between flushes: one group (a head + 7 step words)
#define PJD_CHK_BYTES      (2 * PJD_NCHK * 64 * 4)
#define PJD_STAGE_BYTES    (PJD_STAGE_ENTRIES * 2 * 64)
// per wave: checkpoints (sync passes) / entry staging (write pass).  LDS sets the kernel's occupancy; measured in
// profiles/r02_occupancy.md: more LDS per workgroup costs throughput at once, and 2 waves per workgroup with 2 KB wave areas
// (4 checkpoints, 16 staged entries) measured best with batches in flight (+1 % on the default input, +5 % on the lighter one
// against 4 waves with 4 KB areas), equal within noise for one batch at a time.
#define PJD_WAVE_LDS       (PJD_CHK_BYTES > PJD_STAGE_BYTES ? PJD_CHK_BYTES : PJD_STAGE_BYTES)
// per wave: the phase table -- one 16-byte record per data unit of the MCU: what the NEXT unit decodes with (table offsets,
// its own record's address, the DC-sum selectors of its component); a unit's completion is one LDS read instead of ~9 VALU
#define PJD_PHASE_LDS      256      // 16 records (an MCU has at most 4 + 2 = 6 units; sampling 2x2 with three components)
#ifndef PJD_TAIL_PRIO
#define PJD_TAIL_PRIO      1        // waves in their second and later re-sync rounds raise their issue priority (s_setprio), see wave_rounds
#endif
#ifndef PJD_IDCT_PRIO
#define PJD_IDCT_PRIO      0        // issue priority of the back end's waves (0..3)
#endif
// The cooperative walker (pjd_k_huffman.hip, walk_lane): a re-sync round with at most PjdDevImage::walk_max active lanes is finished
// by the whole wave taking the lanes one after the other.  A walk has a start-up cost per lane (a window of the bitstream is fetched),
// a round costs the same whatever the number of lanes, so the threshold grows with the subsequence: 3 lanes per 512 bytes (6 at 1024),
// and at least PJD_WALK_DENSE where chains are long -- subsequences shorter than PJD_WALK_DENSE_MCUS MCUs' worth of this picture's
// stream: lanes rarely merge inside their own subsequence.  Measured in profiles/r03_experiments.md (8 then) and again in round 4 after
// the second landing pad per lane made rounds shorter: 4 / 6 / 8 / 12 / 16 lanes -> 2.56 / 2.54 / 2.62 / 2.88 / 3.11 ms for a batch alone,
// no difference with batches in flight.  PJD_WALK_MAX in the environment overrides it for every picture of a batch (0: never walk).
#define PJD_WALK_LANES(sub_bytes)  (((sub_bytes) * 3u) >> 9)
#define PJD_WALK_DENSE     6
#define PJD_WALK_DENSE_MCUS 6
#define PJD_LUT_BITS       9        // first-level Huffman LUT width
#define PJD_L2_BITS        (16 - PJD_LUT_BITS)    // a second-level table is indexed by the bits after the prefix
#define PJD_L1_BYTES       (4 << PJD_LUT_BITS)   // one first-level table: 512 x u32 (low half: the symbol; high half: the symbol PAIR, below)
#define PJD_LUT_LDS_MAX    (6 * PJD_L1_BYTES + 8192)  // decode tables of one table set in LDS; larger -> exact kernel
#define PJD_MAX_TABLES     6        // distinct Huffman tables one image can reference (3 DC + 3 AC)
#ifndef PJD_GENS
#define PJD_GENS           6        // generations of a wave's published exit state (wave_gen): 0 = speculative, 1 = after its own re-sync rounds, g + 1 = after
#endif                              // comparing its entry with generation g of its predecessor (and re-bridging if that differs); the last one is only checked.
                                    // A chain of non-merging lanes that crosses k wave boundaries needs k + 2 generations; never a chain over the whole image.
#define PJD_SYNC_MAX_ITERS 72       // re-sync rounds per wave before giving up (a non-merging chain moves one lane per round)
#define PJD_DC_BLOCK       256      // lanes per DC-prediction scan block
#define PJD_DC_PICTURE_MAX_LANES (8 * PJD_DC_BLOCK)   // single chain: pictures up to this many lanes are settled by one workgroup each (pjd_plan.cpp)
#ifndef PJD_IDCT_THREADS
#define PJD_IDCT_THREADS   256
#endif
#ifndef PJD_IDCT_MAX_DU
#define PJD_IDCT_MAX_DU    96       // data units staged in LDS per IDCT workgroup (<= PJD_IDCT_THREADS); with the group parser (round 3): 72 / 90 / 96 -> 0.59 / 0.53 / 0.525 ms on cfg3
#endif
#define PJD_COEF_SENTINEL  (-32768) // at slot 52 of a baseline picture's dense scratch only: "slot 52 was visited with an explicit 0"
                                    // (zigzag quirk); slot 0 (an absolute DC) and progressive pictures hold -32768 as a value

// Bitstream words of one wave, transposed: row k holds big-endian word k of each of its 64 lanes, counted from
// the lane's own first byte.  A lane reads at most 31 bits past its subsequence, holds three words and keeps two more in flight.
#define PJD_WORD_ROWS(sub_bytes)  ((sub_bytes) / 4 + 8)
// Slots (2 bytes each) of a lane's region.  The write pass emits one 32-bit STEP word per decode step -- one symbol, or the PAIR of
// symbols one table lookup yields (below).  How many steps a lane of `sub_bytes` bytes can take follows from the PICTURE's table set:
// the planner computes the fewest bits per step any stream can sustain with it (Annex-K tables: 3.5 -- a chroma unit of DC 0, one
// +-1 coefficient and an EOB is the pair DC + coefficient, then the EOB: 7 bits in two steps; tables fitted to a dense picture: 4-5;
// without the DC pairs it was 2).
// A region is a sequence of 32-byte GROUPS: one head word + PJD_GROUP_STEPS (7) step words (below), a whole number of groups.
// The write pass still checks the bound (PJD_FLAG_OVERFLOW) before every flush.
#define PJD_GROUP          16       // slots per group = what the write pass stages between two flushes (8 dwords)
#define PJD_GROUP_STEPS    (PJD_GROUP / 2 - 1)
// step_bits_x256: fewest bits of stream per step the picture's table set can be made to sustain, x 256 (pjd_plan.cpp, min_step_bits_x256:
// the minimum mean weight mu of a cycle of the step graph, 17 nodes).  A lane's steps are ONE walk in that graph: cycles (each of mean
// >= mu) and a simple path of at most 16 edges of at least one bit each, so n steps consume at least n * mu - 16 * (mu - 1) bits: n <
// bits / mu + 16.  The bits are the lane's own (steps START inside it) plus what its last step reads past its end (two symbols: < 27 bits,
// at most 6 steps' worth at mu >= 4... 27 at mu = 1), and the pair the lane's end breaks is one more step: 16 + 27 + 1, rounded up.
#define PJD_LANE_SLACK_STEPS 48u
#define PJD_LANE_CAP(sub_bytes, step_bits_x256)   ((((8u * (sub_bytes) * 256u + (step_bits_x256) - 1) / (step_bits_x256) + PJD_LANE_SLACK_STEPS + PJD_GROUP_STEPS - 1) / PJD_GROUP_STEPS + 1u) * PJD_GROUP)

// ---- coefficient entries (lane streams) --------------------------------------------------------
// The write pass turns every decoded Huffman symbol into one 16-bit entry; a STEP word holds the one or two entries of a step:
// low half = entry A, high half = entry B (the second symbol of a pair) or PJD_ENT_NONE.
//   DC symbol            the step's low half IS the DC difference as int16 (12 significant bits); the high half is the unit's first
//                        AC symbol where the table holds that pair (short DC symbols: a flat unit, DC + EOB, is ONE step), else
//                        PJD_ENT_NONE.  Which steps hold a DC difference follows from the position: the first entry of every unit.
//   AC run/size symbol   bits 15..5 = value (11-bit two's complement; 0 for a size-0 symbol such as ZRL), bits 4..0 = run + 1
//                        (1..16): the coefficient lands on slot (next free slot + run)
//   EOB                  0x0000: "run + 1" = 0, value 0 -- completes the unit, stores nothing
//   PJD_ENT_NONE         0x001f ("run + 1" = 31): no entry (only in the high half)
// A unit is [DC][AC ...] up to and including an EOB or the entry that lands on slot 63 (next free slot = 64).  A size-0 symbol
// stores an explicit 0 (reference src/jpeg_scanner.cpp:516-517), which matters at slot 52 only (zigzag quirk).
// Steps are kept in GROUPS of 8 dwords = 32 bytes, the unit the write pass flushes: dword 0 is the group's HEAD, `[units completed
// in this lane before the group's first entry : 24][zigzag slot that entry fills from : 8]` (slot 0: the entry is a unit's DC
// difference; else the AC coefficient lands on slot + run), dwords 1..7 hold 7 steps.  With the head a back-end thread parses its
// group without looking at anything before it (pjd_k_idct_colour_lanes); the head travels in the same 32-byte store as its steps.
// Positions in a lane's region (PjdDevLaneInfo::n_ent, PjdDevMark::ent_off) count 16-bit SLOTS, heads included (always even).
// Round 4: the write pass used to emit one entry per step (one symbol); with the pair tables it takes two symbols in 60 % of
// its steps on dense streams, and a step's two entries travel in one LDS word whatever the other lanes of the wave decoded.
#define PJD_ENT_NONE       0x001fu
#define PJD_ENT_EOB        0x0000u

// ---- image flags (device side) -----------------------------------------------------
#define PJD_IF_STANDARD_RESTART 1u  // restart every RI-th MCU; else the reference's (y*Wr+x)%RI rule
#define PJD_IF_SEQUENTIAL       2u  // routed to the exact one-lane kernel up front
#define PJD_IF_BMP              4u  // output is a BMP file image (else tight RGB8)
#define PJD_IF_STANDARD_ZIGZAG  8u  // zigzag slot 48 -> natural 58, no slot-52 override (PJD_F_STANDARD_ZIGZAG)
#define PJD_IF_PROGRESSIVE      32u // a progressive frame: decoded scan by scan into the dense scratch by pjd_k_progressive (PJD_F_PROGRESSIVE)
#define PJD_IF_ENDS_STREAM      16u // the last restart segment this image (or shard) decodes is the last of its bitstream: running out of
                                    // bits there is the reference's end-of-data error, handled by the parallel decoder itself
#define PJD_IF_SCALE_SHIFT      6   // bits 7..6: log2 of the output scale denominator (PJD_F_SCALE_*): 0 full size, 1..3 = 1/2, 1/4, 1/8
#define PJD_IF_SCALE_MASK       (3u << PJD_IF_SCALE_SHIFT)
#define PJD_IF_PLANAR           256u // output is planar R, G, B (PJD_OUT_RGB8_PLANAR): three planes of out_stride x output rows bytes; a property of
                                     // the whole batch (the planar back-end kernels are launched for it), never together with PJD_IF_BMP

#define PJD_IF_LIBJPEG          512u // PJD_F_LIBJPEG: the picture is libjpeg's (islow IDCT, fancy upsampling, JFIF colour): the back end of pjd_k_backend_std.hip;
                                     // always together with PJD_IF_STANDARD_ZIGZAG and PJD_IF_STANDARD_RESTART
#define PJD_IF_GRAY             1024u // output is one plane (PJD_OUT_GRAY8): out_stride x output rows bytes; a property of the whole batch (the grey
                                     // back-end kernels of pjd_k_backend_gray.hip are launched for it), never together with PJD_IF_BMP or PJD_IF_PLANAR
#define PJD_IF_LJSCALE_SHIFT    11  // bits 12..11: PJD_F_LIBJPEG_SCALE_* of a PJD_IF_LIBJPEG picture, log2 of the denominator (0 full size, 1..3 = 1/2, 1/4,
#define PJD_IF_LJSCALE_MASK     (3u << PJD_IF_LJSCALE_SHIFT)   // 1/8): libjpeg's reduced IDCTs -- the _red kernels of pjd_k_backend_std.hip / _gray.hip.
                                                               // Never together with PJD_IF_SCALE_MASK (the box filter)
// log2 of a picture's output scale denominator, whichever of the two scales it has
#define PJD_IF_OUT_SCALE_LOG(flags) ((((flags) & PJD_IF_SCALE_MASK) >> PJD_IF_SCALE_SHIFT) + (((flags) & PJD_IF_LJSCALE_MASK) >> PJD_IF_LJSCALE_SHIFT))
// Samples a side of a CHROMA unit's IDCT where a luma unit has n (8, 4, 2, 1): libjpeg's rule (jdmaster.c) -- the transform doubles while
// that leaves no more samples than the luma has on either axis.  4:2:0 below full size: 2n, and no upsampling is left; everything else: n.
static inline __host__ __device__ uint32_t pjd_lj_chroma_size(uint32_t n, uint32_t hs, uint32_t vs)
{
    uint32_t cn = n;
    while (cn < 8u && 2u * cn <= hs * n && 2u * cn <= vs * n) cn *= 2u;
    return cn;
}

// status word per image: low 8 bits = PJD_ST_* class, bit 8 = "fast path gave up, needs exact kernel"
#define PJD_STW_NEEDS_EXACT 0x100

// What the parallel decoder found wrong in an image, kept per image and ordered by POSITION in the stream (PjdDevBatch::imstate):
//   err_key   the first entropy-coding error of the true decode (the reference stops there, jpeg_scanner.cpp:470-514; everything
//             decoded before it is kept, the rest of the picture stays undecoded): minimum over the lanes that met one of
//             (bit position of the offending symbol << 32) | (index of its data unit << 4) | (PJD_ST_* class << 1 ... see below);
//             the write pass finds it by itself -- bad symbol, bad size, run past slot 63, end of data -- so such pictures
//             need no second decode
//   flag_pos  bit position (start of the lane, or of the wave's first lane) of the earliest thing the decoder could NOT resolve
//             (PJD_FLAG_*): only that, and only if it lies before the first error and not behind the picture's last unit, sends the
//             picture to the exact kernel
//   end_pos   bit position at which the last unit of the picture ended, published by the unflagged lane whose write pass completed
//             the stream's last segment.  Bytes behind it (padding in front of the EOI) hold nothing the reference decodes: a lane
//             that STARTS behind it has no unit, and what the decoder could not resolve there -- a long run of bytes that never
//             self-synchronises ends as PJD_FLAG_STITCH -- does not count.  A lane that published from a stale entry state lies
//             in a wave that is flagged itself, at or before that lane, so a wrong end_pos never hides a flag
// layout of err_key's low word: bits 31..4 data unit, bits 3..1 PJD_ST_* class, bit 0 = the error is in the unit's DC symbol
struct PjdDevImState {
    unsigned long long err_key;        // ~0: none
    uint32_t flag_pos;                 // ~0: none
    uint32_t end_pos;                  // ~0: none
};

// why the parallel decoder flagged an image (PjdDevBatch::stats[PJD_STAT_FLAG0 + reason], counted per wave)
enum {
    PJD_FLAG_SYMBOL = 0,     // invalid code, size or run outside the baseline limits
    PJD_FLAG_SEGMENT,        // a restart segment ends early / late / off a byte boundary, phase or count mismatch
    PJD_FLAG_NOSYNC,         // re-sync rounds did not converge within PJD_SYNC_MAX_ITERS
    PJD_FLAG_STITCH,         // the entry a wave used is not what its predecessor finally produced
    PJD_FLAG_TIMEOUT,        // a bounded wait on another wave expired, or that wave was poisoned
    PJD_FLAG_OVERFLOW,       // a lane needed more than PJD_LANE_CAP entries
    PJD_FLAG_VERIFY,         // the write pass did not reproduce the synchronised exit state / unit count
    PJD_FLAG_REASONS
};
#define PJD_STAT_FLAG0 4
#define PJD_STAT_ENTRIES 11  // PjdDevBatch::stats[]: entries (= Huffman symbols) the lanes emitted in this decode
#define PJD_STAT_STEPS   14  // step words they took for it (a step holds one symbol or a pair)
#define PJD_STAT_FILL    15  // fullest lane region of the decode: slots written x 1024 / PJD_LANE_CAP of its picture (atomic max)
#define PJD_STAT_WALKS   12  // cooperative walks (a wave taking over its few remaining active lanes), 13: lanes walked in them

struct PjdDevImage {
    uint32_t width, height;
    uint32_t mcux, mcuy, n_mcu;        // MCU grid (MCU = 8*hs x 8*vs pixels)
    uint32_t ncomp, hs, vs;
    uint32_t n_luma;                   // hs*vs
    uint32_t dus_per_mcu;              // n_luma + ncomp - 1
    uint32_t restart_interval;
    uint32_t flags;
    uint32_t ref_mcu_w, ref_mcu_h, ref_mcu_w_real;   // reference Header::mcu_width / mcu_height / mcu_width_real
    uint32_t ecs_len;                  // bytes
    uint64_t ecs_off;                  // into the batch bitstream buffer (16-byte aligned)
    uint64_t dense_base;               // first data unit of this image in the DENSE scratch (exact-kernel path only)
    uint32_t n_du;
    uint32_t image_index;
    uint32_t out_stride;               // bytes per output row of the (scaled) picture, width w = ceil(W / s): BMP 3w + w%4, RGB8 3w, planar and grey w (a plane row)
    uint64_t out_off;                  // into the batch output buffer (256-byte aligned), or the caller's (pjd_batch_bind_output: any offset)
    uint32_t seg_base, n_seg;          // into PjdDevSegment[]
    uint32_t lane_base, n_lane;        // into PjdDevSub[] (global lane index)
    uint32_t hwave_base, n_hwave;      // Huffman waves of this image (global wave index)
    uint32_t iwg_base, n_iwg;          // IDCT workgroups (= coefficient ranges) of this image
    uint32_t idct_mcus;                // MCUs per IDCT workgroup
    uint32_t first_mcu, last_mcu;      // MCU range this shard decodes: [first_mcu, last_mcu)
    uint32_t tset;                     // table set (PjdDevTset) of this image
    uint32_t sub_bytes;                // subsequence size of THIS image (<= the batch's, which sizes word rows and lane regions)
    uint8_t  tbl_slot[3][2];           // [component][0=DC,1=AC] -> table slot 0..n_tables-1 of the set
    uint8_t  walk_max;                 // re-sync rounds with at most this many active lanes are walked cooperatively (0: never)
    uint8_t  pad_;
    uint32_t pscan_base, n_pscan;      // progressive frames: their scans in PjdDevBatch::pscans
    uint32_t lane_cap;                 // slots of one lane region of THIS image: PJD_LANE_CAP(sub_bytes, min symbol bits of its table set)
    uint32_t plane_off256;             // PJD_IF_LIBJPEG: the picture's component planes in the batch's plane buffer, in units of 256 bytes (pjd_k_backend_std.hip)
    uint64_t ent_base;                 // first slot of lane `lane_base` in PjdDevBatch::ent; lane q of the image owns [ent_base + (q - lane_base) * lane_cap, + lane_cap)
};

// raw Huffman table as shipped by the host (reference HuffmanTable, jpeg.h:129-134)
struct PjdDevHuffRaw {
    uint8_t offsets[17];
    uint8_t symbols[162];
    uint8_t is_ac;
};                                     // 180 bytes

// One scan of a progressive frame (pjd_scan_desc): what it refines, with which tables, and where its bytes lie
struct PjdDevScan {
    uint64_t ecs_off;                  // into the batch bitstream buffer
    uint32_t ecs_len;
    uint32_t restart_interval;         // in MCUs of THIS scan
    uint8_t  n_comp, comp[3];
    uint8_t  ss, se, ah, al;
    PjdDevHuffRaw table[3];            // per scan component: DC table (ss == 0) or AC table
};

// One table set = the deduplicated Huffman tables of an image; images with identical sets share one (a batch of
// files written with the Annex-K tables has a single set), and so can the waves of one Huffman workgroup.
// Decode-ready form, built on the device by pjd_k_build_tables, one blob per set:
//   [table 0 L1][table 1 L1]...[table n-1 L1][second-level regions: 2 .. 128 u16 per long prefix, table by table]
// L1 is indexed by the next PJD_LUT_BITS (9) bits and holds 32-bit entries; the LOW half describes the symbol that starts there --
// every field the per-symbol loops need comes out with one AND or one bit-field extract, and the zigzag bookkeeping is ONE
// subtraction (see PJD_LUT_ADV):
//   bits  4..0  bits consumed by the symbol (code length + value bits), 1..27; 0 marks a pointer entry (below)
//   bits 10..5  "advance": run + 1 for an AC run/size symbol, 1 for a DC symbol, 32 for an EOB
//   bit  11     EOB (AC tables only).  Bits 11..5 read as ONE 7-bit number are the slots the symbol uses up -- 96 for an EOB,
//               more than any unit has left -- so "63 - slot" minus that number going negative is "the unit is complete";
//               a run/size symbol that lands past slot 63 (an error in the reference, jpeg_scanner.cpp:500) leaves -16..-2 there,
//               an EOB -96..-34, a unit that ends exactly on slot 63 leaves -1: the write pass tells them apart with one minimum.
//               The low five bits of that number are the "run + 1" field of the symbol's lane-stream entry (0 for an EOB)
//   bits 15..12 value bits (size) 0..11, or an invalid symbol (the code alone is consumed):
//               14 = the reference's "symbol 0xFF": no code starts with these bits (then 16 bits are consumed, as its
//                    get_next_symbol does), or the table really holds the symbol 0xFF (jpeg_scanner.cpp:470,490)
//               15 = a DC size > 11 / an AC size > 10 (jpeg_scanner.cpp:474,506)
//   pointer entry (bits 4..0 == 0): codes with this 9-bit prefix P are longer than 9 bits.  The prefix has a second-level table
//               of 2^k u16 entries of the form above (code lengths 10 .. 9 + k), 9 + k the LONGEST code under P (k = 1..7),
//               indexed by the top k of the seven bits that follow the prefix.  Bits 9..5 = 32 - k: the right shift that leaves
//               that index of the window moved up by the prefix (PJD_LUT_PTR_SHIFT); bits 31..16 = BYTE offset of the table,
//               relative to the blob (PJD_LUT_PTR_BYTES: a pointer entry has no pair, the lookup overwrites the high half).
// The HIGH half of an L1 entry describes the PAIR "this symbol and the one after it" where the 9 bits hold the first symbol whole
// (code and value bits), it is a valid run/size symbol (not an EOB) or a valid DC symbol, and the rest of the 9 bits determine the next
// code (any valid AC symbol, an EOB too; its value bits may lie outside) -- for a DC table: a code of the AC table its components
// decode with (PjdDevTset::pair_ac):
//   bits 20..16 bits consumed by both symbols (2..27+; the symbol's own: no pair here)        bits 27..21 slots both use up (advance 1 + advance 2)
//   bits 31..28 value bits (size) of the second symbol (its value is the last `size` of the bits both consume)
// Every pass takes a pair in ONE step when the first symbol neither completes the unit nor reaches the next checkpoint /
// subsequence end: dense streams average 5 bits per symbol, 60 % of the steps there are pairs (profiles/r03_experiments.md).
// Canonical codes keep all long codes in one contiguous range of prefixes [p0, p1), and codes grow with their value: k does not fall
// as P rises, only the last prefix or two of a table hold 15- or 16-bit codes (128 entries), the ones before them need 2 to 8.  The
// second-level region of a table is the tables of its prefixes p0 .. p1 - 1 one after the other, described by the first prefix and the
// first entry of every class k (an empty class starts where the next one does).  The Annex-K set: a blob of 8,784 bytes (at 256 bytes
// per long prefix, the layout before this one and still the accounting that ROUTES a set, pjd_plan.cpp: 11,008).
struct PjdDevTset {
    uint32_t lut_off16;                // blob offset in PjdDevBatch::luts, 16-byte units
    uint32_t lut_bytes;                // multiple of 16
    uint32_t n_tables;
    uint16_t l2_cp[PJD_MAX_TABLES][PJD_L2_BITS];   // table t, class k = 1..7 at [k - 1]: the first 9-bit prefix whose longest code has 9 + k bits (l2_cp[t][0] = p0) ...
    uint16_t l2_ce[PJD_MAX_TABLES][PJD_L2_BITS];   // ... and the u16 index, relative to the blob, of that prefix's table; prefix P of the class: + ((P - first) << k)
    uint16_t l2_p1[PJD_MAX_TABLES];    // 9-bit prefixes [p0, p1) hold codes longer than PJD_LUT_BITS
    uint8_t  pair_ac[PJD_MAX_TABLES];  // of a DC table: the AC table (slot) every component that uses it decodes with -- its entries hold the pair
                                       // "DC symbol + the unit's first AC symbol" -- or 0xff (none: components disagree)
    uint8_t  pad_[2];
};
#define PJD_LUT_USED(e)  ((e) & 31u)
#define PJD_LUT_ADV(e)   (((e) >> 5) & 127u)      // run + 1; 96 for an EOB
#define PJD_LUT_SIZE(e)  (((e) >> 12) & 15u)
#define PJD_LUT_PAIR_USED(e)  (((e) >> 16) & 31u)  // == PJD_LUT_USED(e): no pair (the pair field then repeats the symbol's used / advance)
#define PJD_LUT_PAIR_ADV(e)   (((e) >> 21) & 127u)
#define PJD_LUT_PAIR_SIZE2(e) ((e) >> 28)
#define PJD_LUT_PTR_SHIFT(e)  (((e) >> 5) & 31u)   // of a pointer entry: 32 - k
#define PJD_LUT_PTR_BYTES(e)  ((e) >> 16)          // ... and the byte offset of the prefix's second-level table
#define PJD_LUT_EOB      0x0800u
#define PJD_LUT_BADSYM   14u
#define PJD_LUT_BADLEN   15u
#define PJD_LUT_ENTRY(used, adv, eob, size)  ((used) | ((adv) << 5) | ((eob) ? PJD_LUT_EOB : 0u) | ((size) << 12))

struct PjdDevSegment {                 // one restart segment
    uint32_t byte_start;               // relative to the image's ecs
    uint32_t byte_end;
    uint32_t first_du;                 // image-relative index of its first data unit
    uint32_t n_du;
};

struct PjdDevSub {                     // one Huffman subsequence (decode lane)
    uint32_t byte_start;               // relative to the image's ecs
    uint32_t seg;                      // global segment index | (1u<<31 if first subsequence of its segment)
};

struct PjdDevHuffWave {                // one Huffman wave: up to 64 consecutive lanes of one image
    uint32_t image;
    uint32_t first_lane;               // global lane index
    uint32_t n_lanes;                  // 1..64
    uint32_t pad_;
};

struct PjdDevHuffWg {                  // one Huffman workgroup: up to PJD_HUFF_WAVES consecutive waves of one table set
    uint32_t first_wave;
    uint32_t n_waves;
    uint32_t tset;
    uint32_t pad_;
};

struct PjdDevIdctWg {                  // one IDCT/colour workgroup = one coefficient range
    uint32_t image;
    uint32_t first_mcu;
    uint32_t n_mcu;
    uint32_t pad_;
};

// One picture GROUP: pictures of similar stream density, decoded by its own chain of launches (entropy decode -> DC predictors ->
// back end) beside the other groups' chains, so that the back end of the light pictures runs while the dense pictures' chains of
// re-sync rounds are still finishing (round 4: one batch alone was entropy-decode tail + the whole back end, one after the other).
#define PJD_MAX_GROUPS 8
struct PjdDevGroup {
    uint32_t hwg_first, hwg_count;     // its Huffman workgroups: a range of PjdDevBatch::hwgs (start order: densest pictures first)
    uint32_t img_first, img_count;     // its pictures: a range of PjdDevBatch::group_images
    uint32_t iwg_first, iwg_count;     // its back-end workgroups: a range of PjdDevBatch::iwg_order
    uint32_t pad_[2];
};

// what a Huffman lane leaves behind for the back end (written at the end of its write pass)
struct PjdDevLaneInfo {
    uint32_t n_ent;                    // slots used in the lane's region (group heads included; two per step word)
    uint32_t first_du;                 // bits 27..0: image-relative index of the data unit the lane's first entry belongs to (a unit may span lanes);
                                       // bit 31: the lane starts a restart segment (DC predictors are zero there)
    uint16_t dc_sum[3];                // sum of the DC differences decoded in this lane, per component (mod 2^16)
    uint16_t pad_;
};
#define PJD_LANE_SEG_FIRST 0x80000000u

// DC predictors at the start of a lane, from the scan over PjdDevLaneInfo::dc_sum (pjd_k_lane_dc_*)
struct PjdDevLaneDc {
    uint16_t dc_in[3];                 // relative to the start of the lane's scan block, or absolute if `abs`
    uint16_t abs;                      // 1: a segment head lies between the block start and this lane
};

// where an IDCT workgroup's first data unit starts in the lane streams (written by the lane that decodes
// that unit's DC symbol)
struct PjdDevMark {
    uint32_t lane;                     // global lane index
    uint32_t ent_off;                  // entry index inside the lane's region
    uint16_t acc[3];                   // DC differences summed over this lane up to (not including) that unit
    uint16_t pad_;
};

// packed decoder state at a subsequence boundary: bit position (relative to the
// image's ecs), data-unit phase within the MCU, zigzag slot
static inline __host__ __device__ uint64_t pjd_pack_state(uint32_t p, uint32_t c, uint32_t z)
{
    return (uint64_t)p | ((uint64_t)c << 32) | ((uint64_t)z << 40);
}

// ---- resize on decode (pjd_batch_set_resize; the arithmetic is normative: include/pjd.h) -------------------------------------
// One axis of the bilinear filter: target sample i of dn, over sn source samples -> the two source samples i0, i1 and the weight w
// of i1 in 1/256 (0..256).  THE implementation: pjd_resize_tap exports it to the host, pjd_k_resize runs it per column and per row.
// sn, dn in 1..65535, i < dn.  Where sn * dn < 2^31 every value fits 32 bits (X < 2 * dn * sn, the remainder times 256 < 2^25) and the
// two divisions are 32-bit ones -- every picture anyone decodes; the 64-bit form is the same arithmetic.  On the device the 64-bit
// form and the top of the 32-bit one (sn = 32768, dn = 65535) are pinned by tests/test_gpu_geometry.py
// (test_resize_at_the_dimension_limits), on the host by tests/test_geometry_cpu.py.
static inline __host__ __device__ void pjd_resize_tap_calc(uint32_t sn, uint32_t dn, uint32_t i, uint32_t &i0, uint32_t &i1, uint32_t &w)
{
    const uint32_t d2 = 2u * dn;
    if ((uint64_t)sn * dn < (1ull << 31)) {
        const uint32_t a = (2u * i + 1u) * sn;                  // X = a - dn, clamped to [0, 2 * dn * (sn - 1)]
        uint32_t X = a > dn ? a - dn : 0u;
        const uint32_t hi = d2 * (sn - 1u);
        X = X < hi ? X : hi;
        i0 = X / d2;
        w = ((X - i0 * d2) * 256u + dn) / d2;
    } else {
        const uint64_t a = (uint64_t)(2u * i + 1u) * sn;
        uint64_t X = a > dn ? a - dn : 0u;
        const uint64_t hi = (uint64_t)d2 * (sn - 1u);
        X = X < hi ? X : hi;
        i0 = (uint32_t)(X / d2);
        w = (uint32_t)(((X - (uint64_t)i0 * d2) * 256u + dn) / d2);
    }
    i1 = i0 + 1u < sn ? i0 + 1u : sn - 1u;
}

// The work list of the resample launch (pjd_k_resize.hip), built by pjd_resize_resolve (pjd_resize_plan.cpp): one record per picture and the prefix
// sum of their TILES.  A tile is PJD_RS_ROWS target rows x PJD_RS_COLS target columns, the work of one wave: lane l makes
// PJD_RS_PX adjacent pixels of every row of the tile.
#define PJD_RS_PX    4
#define PJD_RS_COLS  (64 * PJD_RS_PX)
#define PJD_RS_ROWS  8
#define PJD_RS_WAVES 4                 // waves (tiles) per workgroup
struct PjdDevResize {
    uint64_t src_off;                  // the picture at its decode size in the intermediate buffer (where the back end wrote it)
    uint64_t dst_off;                  // the resized picture in the result buffer (the batch's, or the caller's: any offset)
    uint32_t sw, sh, src_stride;       // source: pixels, and bytes per row (3 * sw interleaved, sw planar: a plane row)
    uint32_t tw, th;                   // target
    uint32_t col_tiles;                // tiles per tile row: ceil(tw / PJD_RS_COLS)
};

// ---- antialiased resize (pjd_batch_set_resize_filter; the arithmetic is normative: include/pjd.h) ----------------------------
// One axis of the widened triangle filter: target sample i of dn over sn source samples -> the first source sample with a weight,
// the number of taps (returned; 1..PJD_AA_MAX_TAPS) and their weights q[0 .. count-1] in 1/65536, which sum to 65536 exactly.  THE
// implementation: pjd_resize_aa_taps exports it, pjd_resize_resolve (pjd_resize_plan.cpp) fills the batch's weight table with it (the kernel
// divides nothing).  sn, dn in 1..65535, i < dn, sn <= 16 * dn.  All in 64 bits: (2 * i + 1) * sn reaches 2^33.
static inline __host__ __device__ uint32_t pjd_resize_aa_taps_calc(uint32_t sn, uint32_t dn, uint32_t i, uint32_t &first, uint32_t *q)
{
    const int64_t S2 = 2 * (int64_t)(sn > dn ? sn : dn), c = (int64_t)(2u * i + 1u) * sn, d2 = 2 * (int64_t)dn;
    const int64_t lo = c - S2;                                 // taps: lo < (2 * j + 1) * dn < c + S2
    first = lo < (int64_t)dn ? 0u : (uint32_t)((lo - dn) / d2) + 1u;
    uint32_t n = 0, best = 0;
    uint64_t R = 0;
    // n < 32 (PJD_AA_MAX_TAPS) never ends the loop where sn <= 16 * dn; it keeps a caller's array safe whatever comes in
    for (int64_t p = (2 * (int64_t)first + 1) * dn; n < 32u && first + n < sn && p < c + S2; p += d2, n++) {
        const int64_t dist = p > c ? p - c : c - p;
        q[n] = (uint32_t)(S2 - dist);                          // r_j, 1..2S
        R += q[n];
        if (q[n] > q[best]) best = n;
    }
    int64_t rest = 65536;
    for (uint32_t k = 0; k < n; k++) {
        q[k] = (uint32_t)(((uint64_t)q[k] * 65536u + R / 2u) / R);
        rest -= q[k];
    }
    q[best] = (uint32_t)((int64_t)q[best] + rest);
    return n;
}

// ---- bicubic resize (pjd_batch_set_resize_filter, PJD_RESIZE_BICUBIC; the arithmetic is normative: include/pjd.h) ----------------
// One axis of Keys' cubic (a = -0.5), widened where the axis shrinks: target sample i of dn over sn source samples -> the first
// source sample of the support, the number of taps (returned; 1..PJD_BICUBIC_MAX_TAPS) and their SIGNED weights q[0 .. count-1] in
// 1/65536, which sum to 65536 exactly.  THE implementation: pjd_resize_bicubic_taps exports it, pjd_resize_resolve fills the
// batch's weight table with it.  HOST ONLY: r_j * 2^17 needs 69 bits at 65535-sample axes, so the quantisation is in 128-bit
// integers; the kernel divides nothing.  sn, dn in 1..65535, i < dn, sn <= 16 * dn.  The raw weights fit 64 bits: T < 2^17, D < 2 * T,
// so every term of the two cubics stays below 2^56 and their sum over 64 taps below 2^62.
static inline uint32_t pjd_resize_bicubic_taps_calc(uint32_t sn, uint32_t dn, uint32_t i, uint32_t &first, int32_t *q)
{
    const int64_t T = 2 * (int64_t)(sn > dn ? sn : dn), c = (int64_t)(2u * i + 1u) * sn, d2 = 2 * (int64_t)dn;
    const int64_t lo = c - 2 * T;                              // taps: lo < (2 * j + 1) * dn < c + 2 * T, whatever their weight
    first = lo < (int64_t)dn ? 0u : (uint32_t)((lo - dn) / d2) + 1u;
    int64_t r[64], R = 0;
    uint32_t n = 0, best = 0;
    // n < 64 (PJD_BICUBIC_MAX_TAPS) never ends the loop where sn <= 16 * dn; it keeps the arrays safe whatever comes in
    for (int64_t p = (2 * (int64_t)first + 1) * dn; n < 64u && first + n < sn && p < c + 2 * T; p += d2, n++) {
        const int64_t D = p > c ? p - c : c - p;
        r[n] = D < T ? 3 * D * D * D - 5 * T * D * D + 2 * T * T * T : -D * D * D + 5 * T * D * D - 8 * T * T * D + 4 * T * T * T;
        R += r[n];
        if (r[n] > r[best]) best = n;
    }
    int64_t rest = 65536;
    for (uint32_t k = 0; k < n; k++) {
        const __int128 num = (__int128)r[k] * 131072 + R, den = 2 * (__int128)R;       // R > 0: the centre lies inside the picture
        __int128 v = num / den;
        if (num % den < 0) v--;                                // floor: round half up for either sign
        q[k] = (int32_t)v;
        rest -= q[k];
    }
    q[best] = (int32_t)(q[best] + rest);
    return n;
}

// What the antialiased launch (pjd_k_resize_aa_body.h; the bicubic one likewise) reads beside the work list of the bilinear one: per picture, where the tables of
// its two axes start in the batch's weight table (in words) and how many taps a row of each holds.  The table of one axis (sn -> dn,
// shared by every picture and axis with that pair): dn head words `first | count << 16`, then taps x dn weights, TAP-MAJOR
// (weight t of target sample i at dn + t * dn + i; 0 from `count` on), so that the lanes of a wave read adjacent words.
struct PjdDevResizeAA {
    uint32_t x_tab, x_taps;
    uint32_t y_tab, y_taps;
};

// the LDS a tile needs for a row segment of `span` source pixels (the host sizes the launch with it, the kernel lays its segment out with it)
// nc: the channels of a planar picture (3, or 1 for a grey batch: one plane segment)
static inline __host__ __device__ uint32_t pjd_resize_aa_lds(uint32_t span, bool planar, uint32_t nc = 3u) { return planar ? nc * ((span + 6u) & ~3u) : (3u * span + 6u) & ~3u; }

// ---- source windows (pjd_batch_set_resize_window; the arithmetic is normative: include/pjd.h) -----------------------------------
// What the windowed launches (pjd_k_resize.hip, WIN) read beside the work list: per picture the window with every default resolved
// (w, h >= 1; vw, vh >= 1; ox + tw <= vw, oy + th <= vh).  The taps of target column i are those of index ox + i' over (w, vw), i' = i
// or tw - 1 - i with PJD_RW_HFLIP, and they address source columns from x on; rows likewise without the mirror.  PjdDevResize keeps
// the whole picture (sh is the plane stride of a planar source) and the delivered target.  With the antialiased filter the tables
// of PjdDevResizeAA are those of the axes (w, vw) and (h, vh): vw and vh are their row lengths.
struct PjdDevResizeWin {
    uint32_t x, y, w, h;
    uint32_t vw, vh;
    uint32_t ox, oy;
    uint32_t flags;                    // PJD_RW_HFLIP; with an orientation (below) PJD_RWI_*
    uint32_t pad_;
};

// ---- orientation (pjd_batch_set_orientation; the arithmetic is normative: include/pjd.h) ----------------------------------------
// D = H^h(V^v(T^t(Q))), Q the picture the resample computes (tw x th of PjdDevResize, which for t = 1 is the delivered picture's
// height x width).  The kernels built with ORI read it from the flags of the picture's window record, already resolved into what
// they do (pjd_orient_flags): bit 0 mirrors the column TAP index (the bit PJD_RW_HFLIP has: the two compose by exclusive-or),
// PJD_RWI_YMIRROR mirrors the position at which a row of Q is stored, PJD_RWI_TRANSPOSE stores Q's columns as D's rows.
//   t = 0:  D[i][j] = Q[v ? th-1-i : i][h ? tw-1-j : j]      -> tap mirror h, store mirror v
//   t = 1:  D[i][j] = Q[h ? th-1-j : j][v ? tw-1-i : i]      -> tap mirror v, store mirror h (D has tw rows of th samples)
#define PJD_RWI_XMIRROR   1u
#define PJD_RWI_YMIRROR   2u
#define PJD_RWI_TRANSPOSE 4u
// the bits (t, v, h) of an EXIF orientation 1..8 (the table of include/pjd.h): t << 2 | v << 1 | h
static inline uint32_t pjd_orient_tvh(uint32_t o)
{
    static const uint8_t tvh[8] = {0, 1, 3, 2, 4, 5, 7, 6};
    return tvh[(o - 1u) & 7u];
}
// ... and the flags the kernels read for it (to be combined with the window's PJD_RW_HFLIP by exclusive-or)
static inline uint32_t pjd_orient_flags(uint32_t o)
{
    const uint32_t b = pjd_orient_tvh(o), t = b >> 2, v = (b >> 1) & 1u, h = b & 1u;
    return t ? PJD_RWI_TRANSPOSE | (v ? PJD_RWI_XMIRROR : 0u) | (h ? PJD_RWI_YMIRROR : 0u) : (h ? PJD_RWI_XMIRROR : 0u) | (v ? PJD_RWI_YMIRROR : 0u);
}

// the window of a picture that has none: all of it, to exactly its target.  A plain launch is the windowed one with this window (the
// kernel bodies fold it away at compile time; the host sizes the LDS of a batch without windows with it)
static inline __host__ __device__ PjdDevResizeWin pjd_resize_win_identity(const PjdDevResize &r)
{
    return PjdDevResizeWin{0, 0, r.sw, r.sh, r.tw, r.th, 0, 0, 0, 0};
}

// the tap indices of the two ends of a tile's columns [c0, c1] of a windowed picture, lowest first: the staged segment runs from the
// first tap of `lo` to the last tap of `hi` (the host sizes the LDS with it, the kernel stages with it)
static inline __host__ __device__ void pjd_resize_win_ends(const PjdDevResizeWin &w, uint32_t tw, uint32_t c0, uint32_t c1, uint32_t &lo, uint32_t &hi)
{
    const bool flip = (w.flags & 1u) != 0;
    lo = w.ox + (flip ? tw - 1u - c1 : c0);
    hi = w.ox + (flip ? tw - 1u - c0 : c1);
}

// ---- pad on decode (pjd_batch_set_resize_pad; normative: include/pjd.h) --------------------------------------------------------------
// What the kernels built with PAD (pjd_k_resize.hip) and the border kernel read beside the work list: per picture the delivered CANVAS
// and where the content rectangle lies in it, all in the delivered picture's coordinates (no orientation permutes them).  PjdDevResize
// keeps the CONTENT as its target (tw x th, Q's where transposed): tiles, taps and mirror extents are the content's, while the row
// length, the plane and the origin of every store are the canvas's.  A picture with an all-zero pad has cw == W, ch == H, left == top == 0.
struct PjdDevResizePad {
    uint32_t W, H;                     // the canvas: out_w x out_h of pjd_batch_set_resize
    uint32_t left, top;                // the content's first column and row
    uint32_t cw, ch;                   // the content: W - left - right by H - top - bottom, each >= 1
    uint32_t pad_[2];
};
// the constants of the border kernel: the fill as twelve bytes of a canvas row.  Planar: d[c] is channel c's element repeated over a
// dword.  Interleaved: d[0..2] are the first twelve bytes of a row of fill (R G B R ... in elements of 1, 2 or 4 bytes; 12 is a
// multiple of every pixel size).  Made on the host by pjd_pad_fill (pjd_resize_plan.cpp).
struct PjdPadFill { uint32_t d[3]; };
// the dword of fill at byte j of a canvas line (any j: an aligned ADDRESS need not be an aligned offset): four bytes of the pattern of
// period 12 from j % 12 on.  p0..p2: d[0..2] interleaved, channel c's d[c] three times planar.
static inline __host__ __device__ uint32_t pjd_pad_fill_dword(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t j)
{
    const uint32_t m = j % 12u, q = m >> 2, sh = 8u * (m & 3u);
    const uint32_t lo = q == 0u ? p0 : q == 1u ? p1 : p2, hi = q == 0u ? p1 : q == 1u ? p2 : p0;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// ---- normalised float output (pjd_batch_set_normalize; the arithmetic is normative: include/pjd.h) ---------------------------
// The fma stage of one sample: the exact value of v * scale + bias rounded ONCE to binary32, to nearest even.  THE implementation:
// pjd_normalize_value exports it to the host (where it is libm's fmaf unless the target has the instruction), the epilogue of
// pjd_k_resize_norm runs it per sample (v_fma_f32, or v_fma_mix*_f16 where the conversion to binary16 follows at once).  Written with
// the builtin so that the result does not depend on the contraction flags of a build.
static inline __host__ __device__ float pjd_normalize_f32(uint32_t v, float scale, float bias) { return __builtin_fmaf((float)v, scale, bias); }
// bytes per element of a PJD_DT_* value (1 = PJD_DT_F16, 2 = PJD_DT_BF16, 3 = PJD_DT_F32 of include/pjd.h)
#define PJD_DT_SIZE(dt) ((dt) == 3 ? 4u : 2u)
// What a batch was given with pjd_batch_set_normalize, as the launcher of the resample takes it; dtype 0: none (uint8 pictures).
struct PjdNormalize {
    int32_t dtype;
    float scale[3], bias[3];
};

// ---- affine warp (pjd_batch_set_resize_affine; the arithmetic is normative: include/pjd.h) ------------------------------------
// The inverse map of one output in Q40, as the kernels of pjd_k_warp.hip read it beside the output's PjdDevResize (whose col_tiles
// then counts tiles of PJD_WARP_COLS columns): row 0 of the matrix makes X = a00 * (2i + 1) + a01 * (2j + 1) + b0 for target pixel
// (i, j), which is 2 * (u - 1/2) in Q40 -- b0 = 2 * a02 - 2^40 has the half pixel of both grids folded in -- and row 1 makes Y
// likewise.  48 bytes.  Made by pjd_warp_quantise (pjd_resize_plan.cpp), which also holds the limits: |a00|, |a01|, |a10|, |a11| <=
// 2^44 and |a02|, |a12| <= 2^58, so that with 2i + 1 < 2^17 + 2^7 (a lane past the last column or row of a tile still steps) every sum
// stays below 2^62.3 in magnitude and no step of the 64-bit arithmetic wraps.
struct PjdDevWarp {
    int64_t a00, a01, b0;
    int64_t a10, a11, b1;
};
// A tile of the warp launch: one wave, PJD_WARP_LX lanes along a row with PJD_RS_PX adjacent pixels each and 64 / PJD_WARP_LX lanes down,
// every lane PJD_WARP_RPL rows that lie PJD_WARP_LY apart.  32 columns x 32 rows, and one load instruction of the wave covers 32 x 8
// target pixels: its footprint in the source is as compact under a quarter turn as under none, where the resize tile (PJD_WARP_LX 64,
// PJD_WARP_RPL 8: 256 x 8) touches 256 source rows.  Five shapes were measured (profiles/affine_warp.md); both are build options for
// tools/warp_probe.py.
#ifndef PJD_WARP_LX
#define PJD_WARP_LX   8
#endif
#define PJD_WARP_LY   (64 / PJD_WARP_LX)
#ifndef PJD_WARP_RPL
#define PJD_WARP_RPL  4
#endif
#define PJD_WARP_COLS (PJD_WARP_LX * PJD_RS_PX)
#define PJD_WARP_ROWS (PJD_WARP_LY * PJD_WARP_RPL)
#define PJD_WARP_WAVES 4               // waves (tiles) per workgroup
// X (or Y) of target pixel (i, j) from one row of the record.  Unsigned sums: the same bits, and no signed overflow to reason about.
static inline __host__ __device__ int64_t pjd_warp_pos(int64_t a0, int64_t a1, int64_t b, uint32_t i, uint32_t j)
{
    return (int64_t)((uint64_t)a0 * (uint64_t)(2u * i + 1u) + (uint64_t)a1 * (uint64_t)(2u * j + 1u) + (uint64_t)b);
}
// X -> the source position u - 1/2 in 1/256 pixel, rounded to nearest: its floor p0 (may be negative) and the weight w of p0 + 1 in
// 1/256 (0..255).  |X| < 2^62.3, so the position fits 32 bits.
static inline __host__ __device__ void pjd_warp_fix(int64_t X, int32_t &p0, uint32_t &w)
{
    const int32_t f = (int32_t)((X + ((int64_t)1 << 32)) >> 33);
    p0 = f >> 8;
    w = (uint32_t)f & 255u;
}
// THE implementation of a warp tap: pjd_warp_tap exports it to the host, the body of the warp kernels (pjd_k_warp_body.h) runs
// pjd_warp_pos once per row of a lane, steps it by 2 * a00 and 2 * a10 per pixel -- the same sum, term by term -- and calls pjd_warp_fix.
static inline __host__ __device__ void pjd_warp_tap_calc(const PjdDevWarp &m, uint32_t i, uint32_t j, int32_t &x0, int32_t &y0, uint32_t &wx, uint32_t &wy)
{
    pjd_warp_fix(pjd_warp_pos(m.a00, m.a01, m.b0, i, j), x0, wx);
    pjd_warp_fix(pjd_warp_pos(m.a10, m.a11, m.b1, i, j), y0, wy);
}

// ---- colour map (pjd_batch_set_colour; the arithmetic is normative: include/pjd.h) ----------------------------------------------
// The 3 x 4 map of one output in Q16, as the coloured kernels (pjd_k_resize_col*, pjd_k_warp_col) read it beside the output's
// PjdDevResize: q[c][k] = llrint(m[4c + k] * 65536), o[c] = llrint(m[4c + 3] * 65536).  64 bytes, so that a wave reads its record with
// scalar loads of whole lines.  Made by pjd_colour_quantise (pjd_resize_plan.cpp), which also holds the limits: |q| <= 2^20 and
// |o| <= 2^28, so that no sum of pjd_colour_calc wraps: 3 * 255 * 2^20 + 2^28 + 2^15 < 2^31.
#define PJD_COL_IDENTITY 1u            // flags: q is 65536 * I and o is 0 -- the map changes no sample, and the kernels skip it
struct PjdDevColour {
    int32_t q[3][3], o[3];
    uint32_t flags;
    uint32_t pad_[3];
};
// THE implementation of one sample triple: pjd_colour_value exports it to the host, colour_px of pjd_k_resize_store.h runs it per pixel.
// r, g, b are 8-bit samples and |q| <= 2^20: every product has operands within 24 signed bits, so the 32-bit product of the host text
// is the value of the device's 24-bit multiply-add.  half = o[c] + 32768, the rounding add folded in: three multiply-adds, a shift, one
// med3.  Written as instructions on the device, as pjd_mul_i24 of pjd_device_common.h is and for its reason: the compiler does not see
// the range of a weight it loads, and where it is told (a sign extension) it pairs two multiplies with an add instead of chaining
// three multiply-adds, at a register cost that takes a wave per SIMD from pjd_k_resize_col<planar, uint8> (169 VGPRs against 152:
// figures of the compiler's output, not measured times; profiles/colour_matrix.md).  So the host and the device run two texts of
// one arithmetic, and what holds them together is the byte equality of tests/test_gpu_colour.py against tests/colour_model.py, which
// tests/test_colour_cpu.py holds the host text to.
// The weights are wave-uniform (the record of the tile's output): the "s" operands.
static inline __host__ __device__ uint32_t pjd_colour_calc(const int32_t (&q)[3], int32_t half, uint32_t r, uint32_t g, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t s = half;
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(s) : "s"(q[0]), "v"(r));
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(s) : "s"(q[1]), "v"(g));
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(s) : "s"(q[2]), "v"(b));
    s >>= 16;
#else
    const int32_t s = (q[0] * (int32_t)r + q[1] * (int32_t)g + q[2] * (int32_t)b + half) >> 16;
#endif
    return (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s);
}

// ---- Gaussian blur (pjd_batch_set_blur; the arithmetic is normative: include/pjd.h) ----------------------------------------------
// One output of the blur launch (pjd_k_blur.hip), made by pjd_resize_resolve: U, the uint8 output the resample (or warp) launch of a
// blurred batch wrote into the batch's blur intermediate at src_off, in the batch's layout; the final range at dst_off in the result
// buffer; the taps at taps[tap_off .. tap_off + ksize).  Row 0 of the table is the one tap {65536}, which a record flagged
// PJD_BLUR_IDENTITY reads whatever its ksize (no blur asked for, or a table whose only non-zero tap is the centre): the same arithmetic
// with r = 0, which is the copy.  40 bytes.
#define PJD_BLUR_IDENTITY 1u
struct PjdDevBlur {
    uint64_t src_off, dst_off;
    uint32_t tw, th;
    uint32_t ksize, tap_off;           // as asked for (0: none); the first tap in the table
    uint32_t flags;
    uint32_t col_tiles;                // tiles per tile row: ceil(tw / PJD_BLUR_COLS)
};
// A tile of the blur launch: one workgroup of PJD_BLUR_THREADS, PJD_BLUR_COLS x PJD_BLUR_ROWS samples of one output, a thread
// PJD_RS_PX adjacent pixels of two adjacent rows (pjd_k_blur_body.h)
#define PJD_BLUR_COLS    64
#define PJD_BLUR_ROWS    32
#define PJD_BLUR_THREADS 256
// the LDS of a tile with radius r, ONE channel at a time: the staged bytes (tile + halo, the row pitch a multiple of 4), the row samples
// as 16-bit words, and the finished bytes of all nc channels
static inline __host__ __device__ uint32_t pjd_blur_pitch(uint32_t r) { return (PJD_BLUR_COLS + 2u * r + 3u) & ~3u; }
static inline __host__ __device__ uint32_t pjd_blur_lds(uint32_t r, uint32_t nc)
{
    return (PJD_BLUR_ROWS + 2u * r) * (pjd_blur_pitch(r) + 2u * PJD_BLUR_COLS) + nc * PJD_BLUR_ROWS * PJD_BLUR_COLS;
}
// THE border rule (reflect, include/pjd.h): n in 1..65535, any 32-bit i -- the kernel asks for -31 .. n + 30, which is several periods
// where n is small, so the general case folds by remainder.  pjd_blur_index exports it (its 64-bit i reduced by the period first).
static inline __host__ __device__ uint32_t pjd_blur_index_calc(uint32_t n, int32_t i)
{
    if ((uint32_t)i < n) return (uint32_t)i;               // inside: every sample of an interior tile
    if (n == 1u) return 0u;
    const int32_t p = 2 * ((int32_t)n - 1);
    int32_t m = i % p;
    if (m < 0) m += p;
    return (uint32_t)(m < (int32_t)n ? m : p - m);
}
