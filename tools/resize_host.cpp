// resize_host.cpp -- the bodies of the resample kernels (pim-jpeg-decoder_amd/csrc/pjd_k_resize_body.h and pjd_k_resize_aa_body.h -- the latter
// once per table-driven filter, FILT --, with
// the stores of pjd_k_resize_store.h) run on the host, thread by thread, under the sanitizers, each with WIN false and true: indexing,
// tile search, the vector and the element store paths at every alignment, window and offset indexing, the mirrored tap index, the
// staged segment of a mirrored tile, all four dword remainders of a segment's first byte in both layouts, the plane stride of a planar
// source whose window is lower than the picture, guard bytes.
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize=alignment -D__host__= -D__device__= -o resize_host
//         tools/resize_host.cpp pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp && ./resize_host
//
// Every record the bodies read -- work list, windows, canvases, prefix sums, weight table, the LDS of the launch, the fill pattern -- is
// made by the product's own resolver (pjd_resize_plan.cpp, compiled in) from a request, as the setters of pjd_api.hip make them: the
// bodies run over the host logic itself.  The expectation takes nothing from those records: it is computed from the case alone.
// Device builtins are replaced by host stand-ins: a lane's row taps are computed directly instead of being read from lane k, a
// barrier is nothing, and a thread stages the whole row segment for itself (PJD_WIN_STAGE_*) into an "LDS" of exactly the size the
// host would give the launch, allocated per thread so that AddressSanitizer sees its end.  The 16-bit conversions of the bodies are
// the host compiler's, so this says nothing about the GPU's (tests/test_gpu_normalize.py does); the expectation makes them bit by bit.
// Every variant (uint8 / fp16 / bf16 / fp32, planar / interleaved, bilinear / antialiased / bicubic) writes two sets of pictures, each into one
// buffer at element-aligned offsets with odd gaps, the buffer itself shifted by 0..3 elements:
//   - plain: 31 pictures (tile edges, ragged right edges, random sizes; the table-driven body skips those that shrink more than 16x)
//     through the WIN = false body, and again through the WIN = true body with the identity window: the same bytes;
//   - windowed: 12 geometries (those of tests/test_gpu_resize_window.py and the four remainders of x) and 10 seeded windows;
//   - oriented: those windows and 16 shapes for the transposed store (all eight rows and ragged row tiles, one column, one row, rows of
//     13 samples) through the ORI bodies, every orientation 1..8 (pjd_batch_set_orientation) under windows, mirrors and offsets; the
//     expectation places Q's samples by the table of include/pjd.h.  The plain set also runs through the ORI body: the same bytes;
//   - padded: the oriented set again, every picture a rectangle of a canvas (pjd_batch_set_resize_pad), through the PAD bodies and then
//     the border kernel's body (pjd_k_resize_border_body.h), every thread of its grid: pads that put the rectangle and the canvas
//     width at every remainder modulo four, on one side only, and none at all (such a picture has no border line).  The expectation
//     is the canvas full of fill with the content written over its rectangle: a border byte left out, a content byte filled over or a
//     byte outside a canvas shows.  The plain set also runs through the PAD body: the same bytes;
//   - coloured: the padded set again with a 3 x 4 colour map per picture (pjd_batch_set_colour), through the COL bodies -- the form a
//     coloured request resolves to.  The expectation applies the arithmetic of include/pjd.h in 64 bits to each triple; the border
//     stays the fill as given.  Identity maps (the skipped branch), a permutation, both saturating extremes, the limits.
// The source holds every picture back to back with NO padding between them beyond what rounds the buffer to a dword (the kernels
// stage whole dwords): a read outside a window that mattered would change the result, a read outside the buffer is a sanitizer
// report.  The expectation is a plain per-pixel loop over the arithmetic of include/pjd.h -- the tap inlines with a shifted index;
// the bytes between the pictures are compared too.  The bicubic variants run the same body text with FILT = PJD_RESIZE_BICUBIC: signed
// weights, up to 64 taps an axis (a 16x shrink is among the pictures), results that clamp at both ends on this random source.  Prints ALL EQUAL.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
#define __restrict__
#include "../include/pjd.h"
#include "../pim-jpeg-decoder_amd/csrc/pjd_internal.h"
#include "../pim-jpeg-decoder_amd/csrc/pjd_resize_plan.h"
struct Dim { uint32_t x; };
static thread_local Dim threadIdx, blockIdx;
static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xffffff) * (b & 0xffffff); }
static inline int32_t sext24(int32_t a) { return (int32_t)((uint32_t)a << 8) >> 8; }
static inline int32_t __mul24(int32_t a, int32_t b) { return (int32_t)(uint32_t)((int64_t)sext24(a) * sext24(b)); }   // the low 32 bits of the product of the low 24
static inline void __syncthreads() {}
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_store.h"
#define __builtin_amdgcn_readfirstlane(x) (x)
static inline uint32_t emu_tap(uint32_t sn, uint32_t dn, uint32_t i) { uint32_t y0, y1, wy; pjd_resize_tap_calc(sn, dn, i, y0, y1, wy); return y0 | (wy << 16); }
#define __builtin_amdgcn_readlane(p, k) emu_tap(w.h, w.vh, w.oy + (row0 + (k) < r.th ? row0 + (k) : r.th - 1))
#define PJD_WIN_STAGE_FIRST 0u
#define PJD_WIN_STAGE_STEP  1u

template <bool PLANAR, int DT, bool WIN, bool ORI, bool PAD, bool COL>
static void thread_bilinear(const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const PjdDevResizeWin *win, const PjdDevResizePad *pad,
                            const PjdDevColour *colour, const uint32_t *tile_prefix, uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
    constexpr int NC = 3;                                  // the kernels' channel count: three-channel pictures here
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_body.h"
}

template <bool PLANAR, int DT, bool WIN, bool ORI, bool PAD, bool COL, int FILT>
static void thread_aa(uint32_t *seg, const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const PjdDevResizeWin *win, const PjdDevResizePad *pad,
                      const PjdDevColour *colour, const uint32_t *tile_prefix, uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *aa, const uint32_t *tab, uint32_t lds_bytes,
                      const NormArgs nz)
{
    constexpr int NC = 3;                                  // the kernels' channel count: three-channel pictures here
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_aa_body.h"
}

// one thread of the border kernel (pjd_k_resize_border): lane `lane` of the wave that has canvas line `line`
static void thread_border(uint32_t lane, uint32_t line, uint8_t *dst, const PjdDevResize *recs, const PjdDevResizePad *pad, const uint32_t *line_prefix,
                          uint32_t n_images, uint32_t n_lines, uint32_t planar, uint32_t es, const PjdPadFill fill)
{
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_border_body.h"
}

// the expectation's own conversions to binary16 and bfloat16, round to nearest even
static uint16_t f16bits(float f)
{
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (a < 0x38800000u) {
        const uint32_t e = a >> 23;
        if (e < 102u) return (uint16_t)sign;
        const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return (uint16_t)(sign | q);
    }
    const uint32_t r = a - 0x38000000u;
    uint32_t q = r >> 13; const uint32_t rem = r & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) q++;
    if (q > 0x7c00u) q = 0x7c00u;
    return (uint16_t)(sign | q);
}
static uint16_t bf16bits(float f) { uint32_t b; memcpy(&b, &f, 4); b += 0x7fffu + ((b >> 16) & 1u); return (uint16_t)(b >> 16); }

struct Case { uint32_t sw, sh, tw, th; PjdDevResizeWin w; uint32_t o = 1; uint32_t pad[4] = {0, 0, 0, 0}; };   // o: the orientation (oriented set), tw x th then Q's target; pad: left, top, right, bottom of the delivered canvas (padded set)

// the bits t << 2 | v << 1 | h of an orientation, written out from the table of include/pjd.h (not pjd_orient_tvh: that is under test)
static uint32_t tvh_of(uint32_t o) { return o == 1 ? 0u : o == 2 ? 1u : o == 3 ? 3u : o == 4 ? 2u : o == 5 ? 4u : o == 6 ? 5u : o == 7 ? 7u : 6u; }

static std::vector<Case> plain_cases(unsigned seed, bool aa)
{
    std::vector<Case> all = {{61,45,1,1},{61,45,5,9},{88,56,256,8},{88,56,257,9},{80,96,259,3},{33,70,7,17},{61,45,61,45},{88,56,88,56},{17,9,300,2},{1,1,9,9},{300,1,3,5}}, out;
    srand(seed);
    for (int k = 0; k < 20; k++) all.push_back({(uint32_t)(1 + rand() % 120), (uint32_t)(1 + rand() % 120), (uint32_t)(1 + rand() % 300), (uint32_t)(1 + rand() % 300)});
    for (Case &c : all) {
        PjdDevResize r{}; r.sw = c.sw; r.sh = c.sh; r.tw = c.tw; r.th = c.th;
        c.w = pjd_resize_win_identity(r);
        if (!aa || (c.sw <= 16 * c.tw && c.sh <= 16 * c.th)) out.push_back(c);
    }
    return out;
}

static std::vector<Case> window_cases(unsigned seed)
{
    // x, y, w, h, vw, vh, ox, oy, flags: the geometry of tests/test_gpu_resize_window.py and the four remainders of x
    std::vector<Case> cases = {
        {600, 40, 259, 5, {1, 2, 597, 35, 259, 5, 0, 0, 0, 0}}, {600, 40, 259, 5, {2, 2, 597, 35, 259, 5, 0, 0, 1, 0}},
        {600, 40, 259, 5, {3, 2, 597, 35, 259, 5, 0, 0, 0, 0}}, {600, 40, 259, 5, {4, 2, 596, 35, 259, 5, 0, 0, 1, 0}},
        {200, 120, 4, 4, {100, 40, 64, 64, 4, 4, 0, 0, 0, 0}},
        {300, 20, 270, 9, {0, 0, 300, 20, 600, 20, 250, 3, 0, 0}}, {300, 20, 270, 9, {0, 0, 300, 20, 600, 20, 250, 3, 1, 0}},
        {61, 45, 50, 33, {0, 0, 21, 15, 50, 33, 0, 0, 0, 0}}, {61, 45, 50, 33, {40, 30, 21, 15, 50, 33, 0, 0, 0, 0}},
        {40, 300, 5, 131, {3, 7, 30, 290, 5, 131, 0, 0, 1, 0}},
        {33, 70, 9, 7, {5, 9, 1, 1, 9, 7, 0, 0, 1, 0}},
        {61, 45, 61, 45, {0, 0, 61, 45, 61, 45, 0, 0, 0, 0}}};
    srand(seed);
    for (int k = 0; k < 10; k++) {
        Case c;
        c.sw = 1 + rand() % 150; c.sh = 1 + rand() % 90;
        c.w.w = 1 + rand() % c.sw; c.w.h = 1 + rand() % c.sh; c.w.x = rand() % (c.sw - c.w.w + 1); c.w.y = rand() % (c.sh - c.w.h + 1);
        c.w.vw = std::max<uint32_t>(1 + rand() % 300, (c.w.w + 15) / 16); c.w.vh = std::max<uint32_t>(1 + rand() % 40, (c.w.h + 15) / 16);
        c.tw = 1 + rand() % c.w.vw; c.th = 1 + rand() % c.w.vh; c.w.ox = rand() % (c.w.vw - c.tw + 1); c.w.oy = rand() % (c.w.vh - c.th + 1);
        c.w.flags = rand() & 1; c.w.pad_ = 0;
        cases.push_back(c);
    }
    return cases;
}

// the oriented set: the windowed one and shapes that take the transposed store's paths (all eight rows and ragged, one column, one
// row, D rows of 13 samples: every alignment), each case with the orientation 1 + (index % 8) and so every orientation with windows,
// mirrors and offsets under it
static std::vector<Case> oriented_cases(unsigned seed)
{
    std::vector<Case> cases = window_cases(seed);
    for (Case c : std::vector<Case>{{61, 45, 259, 13}, {45, 300, 5, 259}, {20, 20, 8, 8}, {9, 9, 1, 1}, {9, 20, 1, 9}, {20, 9, 9, 1}, {88, 56, 24, 16}, {61, 45, 259, 13},
                                    {88, 56, 40, 32}, {61, 45, 13, 259}, {88, 56, 16, 24}, {61, 45, 259, 13}, {30, 30, 8, 16}, {61, 45, 259, 13}, {30, 30, 16, 8}, {61, 45, 259, 13}}) {
        PjdDevResize r{}; r.sw = c.sw; r.sh = c.sh; r.tw = c.tw; r.th = c.th;
        c.w = pjd_resize_win_identity(r);
        cases.push_back(c);
    }
    for (size_t i = 0; i < cases.size(); i++) cases[i].o = 1 + (uint32_t)((i + i / 8) % 8);
    return cases;
}

// the padded set: the oriented one, every picture a rectangle of a canvas.  The pads walk through every remainder of left and of the
// canvas width modulo four; every fifth picture has none (no border line of its own in a mixed launch), the others before it a
// pad on one side only, in turn
static std::vector<Case> padded_cases(unsigned seed)
{
    std::vector<Case> cases = oriented_cases(seed);
    for (size_t i = 0; i < cases.size(); i++) {
        const uint32_t k = (uint32_t)i, full[4] = {1 + k % 7, k % 4, (3 * k + 2) % 6, (k / 2) % 5};
        for (int s = 0; s < 4; s++) cases[i].pad[s] = k % 5 == 4 ? 0u : k % 5 == 3 ? (s == (int)(k / 5 % 4) ? 3u + k % 3 : 0u) : full[s];
    }
    return cases;
}

// The colour maps of the coloured set (pjd_batch_set_colour), one per picture: seeded jitters, every fourth the identity (the branch the
// kernels skip the arithmetic under), a permutation, both saturating extremes, and weights and offsets at the limits with mixed signs
static std::vector<PjdColour> colour_cases(size_t n, unsigned seed)
{
    std::vector<PjdColour> cols(n);
    srand(seed + 77);
    for (size_t i = 0; i < n; i++) {
        double *m = cols[i].m;
        for (int k = 0; k < 12; k++) m[k] = k % 5 == 0 ? 1.0 : 0.0;                  // the identity
        if (i % 4 == 0) continue;
        if (i % 11 == 1) { for (int k = 0; k < 12; k++) m[k] = k % 4 == 3 ? 4096.0 : 16.0; continue; }
        if (i % 11 == 2) { for (int k = 0; k < 12; k++) m[k] = k % 4 == 3 ? -4096.0 : -16.0; continue; }
        if (i % 11 == 3) { const double bgr[12] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0}; memcpy(m, bgr, sizeof bgr); continue; }
        if (i % 11 == 5) { for (int k = 0; k < 12; k++) m[k] = k % 4 == 3 ? (k & 4 ? 4096.0 : -4096.0) : ((k + k / 4) & 1 ? -16.0 : 16.0); continue; }
        for (int k = 0; k < 12; k++) m[k] = k % 4 == 3 ? (rand() % 18001 - 9000) / 100.0 : (k % 5 == 0 ? 0.4 + (rand() % 1400) / 1000.0 : 0.0) + (rand() % 1201 - 600) / 1000.0;
    }
    return cols;
}

// mode 0: plain, 1: windowed, 2: oriented (the ORI bodies: windows with an orientation), 3: padded (the PAD bodies and the border kernel's),
// 4: coloured (the padded set with a colour map per picture, through the COL bodies: the form a coloured request resolves to)
template <bool PLANAR, int DT, int FILT>
static int run(int mode, uint32_t misalign_elems, unsigned seed)
{
    const bool coloured = mode == 4;
    const bool windowed = mode != 0, padded = mode == 3 || coloured, oriented = mode == 2 || padded;
    constexpr bool AA = FILT != PJD_RESIZE_BILINEAR;          // a table-driven filter
    const uint32_t ES = DT == 0 ? 1 : PJD_DT_SIZE(DT);
    const std::vector<Case> cases = padded ? padded_cases(seed) : oriented ? oriented_cases(seed) : windowed ? window_cases(seed) : plain_cases(seed, AA);
    const size_t n = cases.size();
    // the request, as a caller of the setters would state it: canvases, pads, orientations, windows, the filter; sources back to back,
    // results at element-aligned offsets with odd gaps
    PjdResizeSpec spec;
    spec.planar = PLANAR;
    spec.pad_set = padded; spec.ori_set = oriented; spec.win_set = windowed; spec.filter_set = true; spec.filter = FILT;
    size_t spos = 0, dpos = misalign_elems * ES;
    std::vector<size_t> doff(n);
    std::vector<uint32_t> cvw(n), cvh(n);                    // the delivered canvases, from the case: Q's target as it is delivered, plus the pad
    for (size_t i = 0; i < n; i++) {
        const Case &c = cases[i];
        const bool tr = oriented && (tvh_of(c.o) >> 2) != 0;
        cvw[i] = (tr ? c.th : c.tw) + c.pad[0] + c.pad[2]; cvh[i] = (tr ? c.tw : c.th) + c.pad[1] + c.pad[3];
        spec.pic.push_back(PjdResizePicture{spos, dpos, c.sw, c.sh, PLANAR ? c.sw : 3 * c.sw});
        spec.out_w.push_back(cvw[i]); spec.out_h.push_back(cvh[i]);
        if (padded) spec.pad.push_back(pjd_resize_pad{c.pad[0], c.pad[1], c.pad[2], c.pad[3]});
        if (oriented) spec.orientation.push_back((uint8_t)c.o);
        if (windowed) spec.win.push_back(pjd_resize_window{c.w.x, c.w.y, c.w.w, c.w.h, c.w.vw, c.w.vh, c.w.ox, c.w.oy, c.w.flags, 0u});
        doff[i] = dpos;
        spos += 3ull * c.sw * c.sh;                        // back to back: a picture's neighbours are other pictures
        dpos += 3ull * cvw[i] * cvh[i] * ES + ES * (2 * (i % 3) + 1);                 // element-aligned odd gaps
    }
    const std::vector<PjdColour> cols = colour_cases(n, seed);
    if (coloured) { spec.colour_set = true; spec.colour = cols; }
    PjdResizeWork work;
    const PjdResizeFault fault = pjd_resize_resolve(spec, work);
    if (!fault.text.empty()) { printf("the resolver refuses the cases: %s\n", fault.text.c_str()); return 1; }
    if (work.form.windowed != windowed || work.form.oriented != oriented || work.form.padded != padded || work.form.coloured != coloured || work.colour.size() != (coloured ? n : 0)) { printf("the resolver chose another form than the cases ask for\n"); return 1; }
    const std::vector<PjdDevResize> &recs = work.recs;
    const std::vector<uint32_t> &prefix = work.tile_prefix, &tab = work.tab;
    const std::vector<PjdDevResizeAA> &aas = work.aa;
    const uint32_t t = work.form.tiles, lds = work.form.lds, n_lines = work.form.lines;
    // the plain set runs through the WIN, ORI and PAD bodies too: with the identity window and a canvas that is the content
    std::vector<PjdDevResizeWin> wins = work.win;
    std::vector<PjdDevResizePad> pads = work.pad;
    std::vector<uint32_t> lprefix = work.line_prefix;
    if (!windowed) {
        lprefix.assign(n + 1, 0u);
        for (size_t i = 0; i < n; i++) { wins.push_back(pjd_resize_win_identity(recs[i])); pads.push_back(PjdDevResizePad{cvw[i], cvh[i], 0, 0, cvw[i], cvh[i], {0u, 0u}}); }
    }
    const size_t src_bytes = (spos + 3) & ~(size_t)3;        // whole dwords are staged: the buffer ends on one, as every allocation does
    uint8_t *src = (uint8_t *)malloc(src_bytes);              // the sanitizer's view of the source is exactly src_bytes
    for (size_t k = 0; k < src_bytes; k++) src[k] = (uint8_t)rand();
    if (((uintptr_t)src & 3u) != 0) { printf("malloc gave an unaligned block\n"); return 1; }
    const size_t dst_bytes = dpos + 256;
    const NormArgs nz = {{0.01712475f, 0.017507f, -0.01742919f}, {-2.117904f, -2.0357144f, 1.8044444f}};
    // the fill of the padded set: the expectation's three elements (the fill byte, or its normalised value), and the pattern of the launch
    const uint8_t fill_u8[3] = {114, 7, 201};
    uint32_t fill_e[3];
    for (int ch = 0; ch < 3; ch++) {
        const float u = fmaf((float)fill_u8[ch], nz.scale[ch], nz.bias[ch]);
        uint32_t b32; memcpy(&b32, &u, 4);
        fill_e[ch] = DT == 0 ? fill_u8[ch] : DT == PJD_DT_F32 ? b32 : DT == PJD_DT_F16 ? f16bits(u) : bf16bits(u);
    }
    PjdNormalize norm{DT, {nz.scale[0], nz.scale[1], nz.scale[2]}, {nz.bias[0], nz.bias[1], nz.bias[2]}};
    const PjdPadFill pf = pjd_pad_fill(norm, PLANAR, fill_u8, nullptr);
    // every thread of the launch, with the WIN = true or the WIN = false body
    auto launch = [&](auto WIN, auto ORI, auto PADDED, auto COLOURED) {
        constexpr bool W = decltype(WIN)::value, O = decltype(ORI)::value, PD = decltype(PADDED)::value, CL = decltype(COLOURED)::value;
        uint8_t *dst = (uint8_t *)aligned_alloc(256, (dst_bytes + 255) & ~(size_t)255); memset(dst, 0xA5, dst_bytes);
        const uint32_t n_threads = AA ? 64 : 64 * PJD_RS_WAVES, n_blocks = AA ? t : (t + PJD_RS_WAVES - 1) / PJD_RS_WAVES;
        for (uint32_t b = 0; b < n_blocks; b++) for (uint32_t th = 0; th < n_threads; th++) {
            blockIdx.x = b; threadIdx.x = th;
            if constexpr (AA) {
                uint32_t *seg = (uint32_t *)malloc(lds ? lds : 4);                   // this thread's "LDS", of the launch's size
                thread_aa<PLANAR, DT, W, O, PD, CL, FILT>(seg, src, dst, recs.data(), W ? wins.data() : nullptr, PD ? pads.data() : nullptr, CL ? work.colour.data() : nullptr, prefix.data(), (uint32_t)n, t, aas.data(), tab.data(), lds, nz);
                free(seg);
            } else {
                thread_bilinear<PLANAR, DT, W, O, PD, CL>(src, dst, recs.data(), W ? wins.data() : nullptr, PD ? pads.data() : nullptr, CL ? work.colour.data() : nullptr, prefix.data(), (uint32_t)n, t, nz);
            }
        }
        if constexpr (PD)                                    // the border kernel behind it: the grid of pjd_launch_resize_border, whole workgroups
            for (uint32_t b = 0; b < (n_lines + PJD_RS_WAVES - 1) / PJD_RS_WAVES; b++) for (uint32_t th = 0; th < 64 * PJD_RS_WAVES; th++)
                thread_border(th & 63u, b * PJD_RS_WAVES + (th >> 6), dst, recs.data(), pads.data(), lprefix.data(), (uint32_t)n, n_lines, PLANAR ? 1u : 0u, ES, pf);
        return dst;
    };
    const std::true_type yes{}; const std::false_type no{};
    // -DPJD_HOST_COLOURED_ONLY builds the coloured set alone (a fifth of the instantiations: tests/test_colour_cpu.py)
#ifdef PJD_HOST_COLOURED_ONLY
    if (!coloured) { printf("built with PJD_HOST_COLOURED_ONLY\n"); return 1; }
    uint8_t *dst = launch(yes, yes, yes, yes);
#else
    uint8_t *dst = coloured ? launch(yes, yes, yes, yes) : padded ? launch(yes, yes, yes, no) : oriented ? launch(yes, yes, no, no) : windowed ? launch(yes, no, no, no) : launch(no, no, no, no);
#endif
    int bad = 0;
    uint32_t clamped = FILT == PJD_RESIZE_BICUBIC ? 0u : 3u;   // bicubic: the final clamp is met at both ends
    uint32_t colour_clamped = coloured ? 0u : 3u;            // coloured: the map's one clamp likewise
#ifndef PJD_HOST_COLOURED_ONLY
    if (!windowed) {                                         // the identity window through the WIN = true body: the same bytes
        uint8_t *again = launch(yes, no, no, no);
        if (memcmp(dst, again, dst_bytes) != 0) { printf("  the identity window through the WIN body gives other bytes\n"); bad++; }
        free(again);
        again = launch(yes, yes, no, no);                        // ... and through the ORI body (orientation 1: no PJD_RWI_* bit)
        if (memcmp(dst, again, dst_bytes) != 0) { printf("  the identity window through the ORI body gives other bytes\n"); bad++; }
        free(again);
        again = launch(yes, yes, yes, no);                       // ... and through the PAD body (no pad: the canvas is the content, no border line)
        if (memcmp(dst, again, dst_bytes) != 0) { printf("  the identity window through the PAD body gives other bytes\n"); bad++; }
        free(again);
    }
#endif
    // the expectation: include/pjd.h, pixel by pixel
    std::vector<uint8_t> want(dst_bytes, 0xA5);
    for (size_t i = 0; i < n; i++) {
        const Case &c = cases[i]; const PjdDevResizeWin &w = c.w; const uint8_t *sp = src + recs[i].src_off;
        const size_t cW = cvw[i], cH = cvh[i], cleft = c.pad[0], ctop = c.pad[1];   // the canvas and the content's origin in it: the case's, not the records'
        if (padded)                                          // the whole canvas is fill; the content is written over its rectangle below
            for (size_t e = 0; e < 3ull * cW * cH; e++) {
                const uint32_t v = fill_e[PLANAR ? e / (cW * cH) : e % 3];
                memcpy(want.data() + doff[i] + e * ES, &v, ES);   // little-endian: the element's low bytes
            }
        auto P = [&](int ch, uint32_t yy, uint32_t xx) -> uint32_t {
            if (xx < w.x || xx >= w.x + w.w || yy < w.y || yy >= w.y + w.h) { printf("the expectation itself left the window\n"); exit(2); }
            return PLANAR ? sp[(size_t)ch * c.sw * c.sh + (size_t)yy * c.sw + xx] : sp[((size_t)yy * c.sw + xx) * 3 + ch];
        };
        for (uint32_t y = 0; y < c.th; y++) for (uint32_t x = 0; x < c.tw; x++) {
          uint32_t v3[3];
          for (int ch = 0; ch < 3; ch++) {
            const uint32_t xi = w.ox + ((w.flags & PJD_RW_HFLIP) ? c.tw - 1 - x : x), yi = w.oy + y;
            uint32_t v;
            if (FILT == PJD_RESIZE_BICUBIC) {
                uint32_t fx, fy; int32_t qx[PJD_BICUBIC_MAX_TAPS], qy[PJD_BICUBIC_MAX_TAPS];
                const uint32_t nx = pjd_resize_bicubic_taps_calc(w.w, w.vw, xi, fx, qx), ny = pjd_resize_bicubic_taps_calc(w.h, w.vh, yi, fy, qy);
                int64_t acc = 0;                             // the expectation in 64 bits: it also says that 32 were enough
                for (uint32_t b = 0; b < ny; b++) {
                    int64_t h = 0;
                    for (uint32_t a = 0; a < nx; a++) h += (int64_t)qx[a] * (int64_t)P(ch, w.y + fy + b, w.x + fx + a);
                    const int64_t h6 = (h + 512) >> 10;
                    if (h != (int32_t)h || h6 >= 32768 || h6 < -32768) { printf("the expectation left the bounds of include/pjd.h\n"); exit(2); }
                    acc += qy[b] * h6;
                }
                if (acc + (1 << 21) != (int32_t)(acc + (1 << 21))) { printf("the expectation left 32 bits\n"); exit(2); }
                const int64_t o = (acc + (1 << 21)) >> 22;
                clamped |= o < 0 ? 1u : o > 255 ? 2u : 0u;
                v = (uint32_t)(o < 0 ? 0 : o > 255 ? 255 : o);
            } else if (AA) {
                uint32_t fx, fy, qx[PJD_AA_MAX_TAPS], qy[PJD_AA_MAX_TAPS];
                const uint32_t nx = pjd_resize_aa_taps_calc(w.w, w.vw, xi, fx, qx), ny = pjd_resize_aa_taps_calc(w.h, w.vh, yi, fy, qy);
                uint32_t acc = 0;
                for (uint32_t b = 0; b < ny; b++) {
                    uint32_t h = 0;
                    for (uint32_t a = 0; a < nx; a++) h += qx[a] * P(ch, w.y + fy + b, w.x + fx + a);
                    acc += qy[b] * ((h + 128u) >> 8);
                }
                v = (acc + (1u << 23)) >> 24;
            } else {
                uint32_t x0, x1, wx, y0, y1, wy;
                pjd_resize_tap_calc(w.w, w.vw, xi, x0, x1, wx); pjd_resize_tap_calc(w.h, w.vh, yi, y0, y1, wy);
                x0 += w.x; x1 += w.x; y0 += w.y; y1 += w.y;
                v = ((256 - wy) * ((256 - wx) * P(ch, y0, x0) + wx * P(ch, y0, x1)) + wy * ((256 - wx) * P(ch, y1, x0) + wx * P(ch, y1, x1)) + 32768) >> 16;
            }
            v3[ch] = v;
          }
          if (coloured) {                                    // include/pjd.h, "colour map", written out in 64 bits: it also says that 32 were enough
              const double *m = cols[i].m;
              uint32_t out[3];
              for (int ch = 0; ch < 3; ch++) {
                  const int64_t sum = (int64_t)std::llrint(m[4 * ch] * 65536.0) * v3[0] + (int64_t)std::llrint(m[4 * ch + 1] * 65536.0) * v3[1] + (int64_t)std::llrint(m[4 * ch + 2] * 65536.0) * v3[2] +
                                      (int64_t)std::llrint(m[4 * ch + 3] * 65536.0) + 32768;
                  if (sum != (int32_t)sum) { printf("the colour expectation left 32 bits\n"); exit(2); }
                  const int64_t o = sum >> 16;
                  colour_clamped |= o < 0 ? 1u : o > 255 ? 2u : 0u;
                  out[ch] = (uint32_t)(o < 0 ? 0 : o > 255 ? 255 : o);
              }
              memcpy(v3, out, sizeof out);
          }
          for (int ch = 0; ch < 3; ch++) {
            const uint32_t v = v3[ch];
            // where Q[y][x] is delivered: D = H^h(V^v(T^t(Q))) of include/pjd.h, D being dw x dh
            const uint32_t b3 = tvh_of(c.o), ot = b3 >> 2, ov = (b3 >> 1) & 1u, oh = b3 & 1u;
            const uint32_t di = ot ? (ov ? c.tw - 1 - x : x) : (ov ? c.th - 1 - y : y), dj = ot ? (oh ? c.th - 1 - y : y) : (oh ? c.tw - 1 - x : x);
            const size_t e = PLANAR ? ((size_t)ch * cH + ctop + di) * cW + cleft + dj : ((ctop + di) * cW + cleft + dj) * 3 + ch;
            uint8_t *o = want.data() + doff[i] + e * ES;
            if (DT == 0) *o = (uint8_t)v;
            else {
                const float u = fmaf((float)v, nz.scale[ch], nz.bias[ch]);
                if (DT == PJD_DT_F32) memcpy(o, &u, 4);
                else { const uint16_t h = DT == PJD_DT_F16 ? f16bits(u) : bf16bits(u); memcpy(o, &h, 2); }
            }
          }
        }
    }
    for (size_t k = 0; k < dst_bytes; k++) if (dst[k] != want[k]) { if (bad < 4) printf("  mismatch at byte %zu got %02x want %02x\n", k, dst[k], want[k]); bad++; }
    uint32_t rem = windowed ? 0u : 0xfu;                     // the windowed set has a segment at every dword remainder
    for (size_t i = 0; i < n; i++) rem |= 1u << ((recs[i].src_off + (PLANAR ? cases[i].w.x : 3 * cases[i].w.x) + (size_t)cases[i].w.y * recs[i].src_stride) & 3u);
    printf("%s %s PLANAR=%d DT=%d misalign=%u: %zu pictures, %u tiles, lds %u, remainders %x, clamps %x: %s\n", FILT == PJD_RESIZE_BICUBIC ? "bicubic  " : AA ? "antialias" : "bilinear ", coloured ? "coloured" : padded ? "padded  " : oriented ? "oriented" : windowed ? "windowed" : "plain   ",
           (int)PLANAR, DT, misalign_elems, n, t, lds, rem, clamped, bad ? "MISMATCH" : "equal, guards intact");
    free(dst); free(src);
    return bad != 0 || rem != 0xf || clamped != 3u || colour_clamped != 3u;
}

template <int FILT>
static int all(int windowed)
{
    int rc = 0;
    for (uint32_t mis : {0u, 1u, 2u, 3u}) {
        rc |= run<true, 0, FILT>(windowed, mis, 1); rc |= run<false, 0, FILT>(windowed, mis, 2);
        rc |= run<true, PJD_DT_F16, FILT>(windowed, mis, 3); rc |= run<false, PJD_DT_F16, FILT>(windowed, mis, 4);
        rc |= run<true, PJD_DT_BF16, FILT>(windowed, mis, 5); rc |= run<false, PJD_DT_BF16, FILT>(windowed, mis, 6);
        rc |= run<true, PJD_DT_F32, FILT>(windowed, mis, 7); rc |= run<false, PJD_DT_F32, FILT>(windowed, mis, 8);
    }
    return rc;
}

// every set; built with -DPJD_HOST_COLOURED_ONLY the coloured set alone (what tests/test_colour_cpu.py builds and runs)
int main()
{
#ifdef PJD_HOST_COLOURED_ONLY
    const int only = all<PJD_RESIZE_BILINEAR>(4) | all<PJD_RESIZE_ANTIALIAS>(4) | all<PJD_RESIZE_BICUBIC>(4);
    printf(only ? "FAILED\n" : "ALL EQUAL\n");
    return only;
#endif
    const int rc = all<PJD_RESIZE_BILINEAR>(4) | all<PJD_RESIZE_ANTIALIAS>(4) | all<PJD_RESIZE_BICUBIC>(4) | all<PJD_RESIZE_BILINEAR>(0) | all<PJD_RESIZE_BILINEAR>(1) | all<PJD_RESIZE_BILINEAR>(2) | all<PJD_RESIZE_BILINEAR>(3) | all<PJD_RESIZE_ANTIALIAS>(0) |
                   all<PJD_RESIZE_ANTIALIAS>(1) | all<PJD_RESIZE_ANTIALIAS>(2) | all<PJD_RESIZE_ANTIALIAS>(3) | all<PJD_RESIZE_BICUBIC>(0) | all<PJD_RESIZE_BICUBIC>(1) |
                   all<PJD_RESIZE_BICUBIC>(2) | all<PJD_RESIZE_BICUBIC>(3);
    printf(rc ? "FAILED\n" : "ALL EQUAL\n");
    return rc;
}
