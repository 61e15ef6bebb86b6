// blur_host.cpp -- the body of the blur kernels (pim-jpeg-decoder_amd/csrc/pjd_k_blur_body.h, with the arithmetic and the stores of
// pjd_k_resize_store.h) run on the host under the sanitizers, in the manner of tools/resize_host.cpp and tools/warp_host.cpp; and the rules
// of the resolver for a blurred request (pjd_resize_plan.cpp) checked beside it.
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize=alignment -D__host__= -D__device__= -o blur_host
//         tools/blur_host.cpp pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp && ./blur_host [dump file]
//
// (clang: the store header uses its vector extensions and 16-bit float types.  tests/test_blur_cpu.py builds and runs it.)
// Every record the body reads -- blur records, prefix sum, tap table -- is made by the product's own resolver from a request, as the
// setter of pjd_api.hip makes it.  A workgroup runs as ONE host thread that takes every item of every phase in turn (PJD_BLUR_T0 /
// _TSTEP of the body), so a barrier is nothing; the LDS is a heap block of exactly the launch's dynamic size, so that a byte beyond it is
// a sanitizer report.  The expectation takes nothing from those records and nothing from pjd_internal.h: plain loops over the text of
// include/pjd.h -- its own taps, the border rule by repeated reflection, the sums in 64 bits with their limits checked.
// The sizes are widths 1, 2, 5, 37, 259 x heights 1, 7, 9, 33, 70, each with 1, 3, 23 and 63 taps, then outputs without a blur and with
// a table that quantises to the identity.  The three uint8 forms take all of them; the nine float forms every seventh, at
// element-aligned offsets with odd gaps, the buffer itself shifted by 0..3 elements.  U lies back to back with NO padding, so a read outside an output
// that mattered changes the result and a read outside the buffer is a sanitizer report; the destination is compared whole, guard
// bytes included.  With a file name the planar uint8 run is written out (per output: w, h, ksize as uint32, sigma as double, U, the result)
// for tests/test_blur_cpu.py to hold against tests/blur_model.py.  Prints ALL EQUAL and the number of failed checks.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
static inline int32_t __mul24(int32_t a, int32_t b) { return (int32_t)(uint32_t)((int64_t)sext24(a) * sext24(b)); }
static inline void __syncthreads() {}
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_store.h"
#define PJD_BLUR_T0    0u
#define PJD_BLUR_TSTEP 1u

template <bool PLANAR, int DT, int NC>
static void group_blur(uint32_t *lds, const uint8_t *src, uint8_t *dst, const PjdDevBlur *recs, const uint32_t *tile_prefix, const uint32_t *taps, uint32_t n_images,
                       uint32_t n_tiles, uint32_t lds_bytes, const NormArgs nz)
{
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_blur_body.h"
}

static int failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failed++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

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

struct Case { uint32_t w, h, ksize; double sigma; };

static std::vector<Case> cases(bool all)
{
    const uint32_t ws[5] = {1, 2, 5, 37, 259}, hs[5] = {1, 7, 9, 33, 70}, ks[4] = {1, 3, 23, 63};
    const double sg[4] = {1.0, 0.8, 2.0, 10.0};
    std::vector<Case> c;
    for (uint32_t w : ws)
        for (uint32_t h : hs)
            for (int k = 0; k < 4; k++) c.push_back(Case{w, h, ks[k], sg[k]});
    c.push_back(Case{37, 33, 0, 0.0});                      // no blur: the copy
    c.push_back(Case{259, 9, 0, 0.0});
    c.push_back(Case{5, 70, 3, 0.1});                       // a table that quantises to the identity
    c.push_back(Case{65, 33, 23, 0.1});                     // ... one sample past a tile edge on each axis
    c.push_back(Case{65, 33, 5, 100.0});                    // a box: every tap a fifth
    c.push_back(Case{64, 32, 63, 1e308});                   // one full tile, the widest box
    if (all) return c;
    std::vector<Case> some;
    for (size_t i = 0; i < c.size(); i++)
        if (i % 7 == 3 || i + 6 >= c.size()) some.push_back(c[i]);
    return some;
}

// include/pjd.h, written out
static void expect_taps(uint32_t ksize, double sigma, int64_t *q)
{
    const int r = (int)(ksize / 2);
    double w[64], t = 0;
    for (int j = 0; j < (int)ksize; j++) { const double d = (j - r) / sigma; w[j] = std::exp(-0.5 * (d * d)); t += w[j]; }
    int64_t sum = 0;
    for (int j = 0; j < (int)ksize; j++) { q[j] = std::llrint(w[j] / t * 65536.0); sum += q[j]; }
    q[r] += 65536 - sum;
}
static uint32_t reflect(int64_t n, int64_t i)              // by repeated reflection about the first and the last sample
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return (uint32_t)i;
}
static void expect_blur(const uint8_t *u, uint32_t w, uint32_t h, uint32_t ksize, double sigma, uint8_t *out)     // one channel, row-major
{
    if (ksize == 0) { memcpy(out, u, (size_t)w * h); return; }
    int64_t q[64];
    expect_taps(ksize, sigma, q);
    const int r = (int)(ksize / 2);
    std::vector<int64_t> h8((size_t)w * h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            int64_t s = 0;
            for (int j = 0; j < (int)ksize; j++) s += q[j] * u[(size_t)y * w + reflect(w, (int64_t)x + j - r)];
            CHECK(s < (1 << 24), "the row sum left 24 bits");
            h8[(size_t)y * w + x] = (s + 128) >> 8;
        }
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            int64_t s = 0;
            for (int j = 0; j < (int)ksize; j++) s += q[j] * h8[(size_t)reflect(h, (int64_t)y + j - r) * w + x];
            CHECK(s + (1 << 23) < ((int64_t)1 << 32), "the column sum left 32 bits");
            out[(size_t)y * w + x] = (uint8_t)((s + (1 << 23)) >> 24);
        }
}

template <bool PLANAR, int DT, int NC>
static void run(uint32_t misalign_elems, unsigned seed, const char *dump)
{
    const uint32_t ES = DT == 0 ? 1 : PJD_DT_SIZE(DT);
    const std::vector<Case> cs = cases(DT == 0);
    const size_t n = cs.size();
    PjdResizeSpec spec;
    spec.planar = PLANAR; spec.channels = NC;
    spec.blur_set = true;
    size_t dpos = misalign_elems * ES;
    std::vector<size_t> doff(n);
    for (size_t i = 0; i < n; i++) {
        const Case &c = cs[i];
        spec.pic.push_back(PjdResizePicture{0, dpos, c.w, c.h, PLANAR ? c.w : 3 * c.w});     // the resample's source is not read here
        spec.out_w.push_back(c.w); spec.out_h.push_back(c.h);
        spec.blur.push_back(pjd_blur{c.sigma, c.ksize, 0});
        doff[i] = dpos;
        dpos += (size_t)NC * c.w * c.h * ES + ES * (2 * (i % 3) + 1);      // element-aligned odd gaps
    }
    PjdResizeWork work;
    const PjdResizeFault fault = pjd_resize_resolve(spec, work);
    CHECK(fault.text.empty(), "the resolver refuses the cases: %s", fault.text.c_str());
    if (!fault.text.empty()) return;
    CHECK(work.form.blurred && work.blur.size() == n && work.blur_prefix.size() == n + 1 && work.blur_prefix[n] == work.form.blur_tiles, "the records of a blurred request");
    CHECK(work.form.blur_lds == pjd_blur_lds(31, NC), "the LDS is that of the largest radius: %u", work.form.blur_lds);
    // U, where the resolver says the resample writes it: the packed layout, exactly as long as it says
    srand(seed);
    uint8_t *src = (uint8_t *)malloc((size_t)work.form.blur_buf_bytes);
    for (size_t k = 0; k < work.form.blur_buf_bytes; k++) src[k] = (uint8_t)rand();
    for (size_t i = 0; i < n; i++) {
        CHECK(work.recs[i].dst_off == work.blur[i].src_off && work.blur[i].dst_off == doff[i], "output %zu: the resample writes U, the blur the result", i);
        CHECK(work.blur[i].src_off + (uint64_t)NC * cs[i].w * cs[i].h <= work.form.blur_buf_bytes, "output %zu lies in the intermediate", i);
        if (i % 5 == 1) memset(src + work.blur[i].src_off, i % 2 ? 255 : 0, (size_t)NC * cs[i].w * cs[i].h);       // black / white
        if (i % 5 == 2) memset(src + work.blur[i].src_off, 77, (size_t)NC * cs[i].w * cs[i].h);                    // constant
    }
    const size_t dst_bytes = dpos + 64;
    uint8_t *dst = (uint8_t *)aligned_alloc(256, (dst_bytes + 255) & ~(size_t)255), *want = (uint8_t *)malloc(dst_bytes);
    memset(dst, 0xA5, dst_bytes); memset(want, 0xA5, dst_bytes);
    const NormArgs nz = {{0.01712475f, 0.017507f, -0.01742919f}, {-2.117904f, -2.0357144f, 1.8044444f}};
    uint32_t *lds = (uint32_t *)aligned_alloc(16, (work.form.blur_lds + 15) & ~15u);
    for (uint32_t b = 0; b < work.form.blur_tiles; b++) {
        memset(lds, 0x5A, work.form.blur_lds);              // nothing of one workgroup reaches the next
        blockIdx.x = b; threadIdx.x = 0;
        group_blur<PLANAR, DT, NC>(lds, src, dst, work.blur.data(), work.blur_prefix.data(), work.blur_taps.data(), (uint32_t)n, work.form.blur_tiles, work.form.blur_lds, nz);
    }
    FILE *df = dump && PLANAR && DT == 0 && NC == 3 && misalign_elems == 0 ? fopen(dump, "wb") : nullptr;
    for (size_t k = 0; k < n; k++) {
        const Case &c = cs[k];
        const size_t px = (size_t)c.w * c.h;
        std::vector<uint8_t> u(px), o(px);
        for (uint32_t ch = 0; ch < (uint32_t)NC; ch++) {
            const uint8_t *s = src + work.blur[k].src_off;
            for (size_t e = 0; e < px; e++) u[e] = PLANAR ? s[ch * px + e] : s[e * 3 + ch];
            expect_blur(u.data(), c.w, c.h, c.ksize, c.sigma, o.data());
            if (c.ksize == 0 || c.ksize == 1 || c.sigma == 0.1) CHECK(o == u, "case %zu is the identity", k);
            if (k % 5 == 2) CHECK(std::count(o.begin(), o.end(), 77) == (long)px, "case %zu: a constant picture stays constant", k);
            for (size_t e = 0; e < px; e++) {
                uint8_t *t = want + doff[k] + (PLANAR ? ch * px + e : e * 3 + ch) * ES;
                if (DT == 0) { t[0] = o[e]; continue; }
                const float f = fmaf((float)o[e], nz.scale[ch], nz.bias[ch]);
                if (DT == PJD_DT_F32) memcpy(t, &f, 4);
                else { const uint16_t hh = DT == PJD_DT_F16 ? f16bits(f) : bf16bits(f); memcpy(t, &hh, 2); }
            }
        }
        if (df) {
            const uint32_t head[3] = {c.w, c.h, c.ksize};
            fwrite(head, 4, 3, df); fwrite(&c.sigma, 8, 1, df);
            fwrite(src + work.blur[k].src_off, 1, 3 * px, df); fwrite(dst + doff[k], 1, 3 * px, df);
        }
    }
    if (df) fclose(df);
    size_t bad = 0, first = 0;
    for (size_t k = 0; k < dst_bytes; k++)
        if (dst[k] != want[k] && !bad++) first = k;
    size_t pic = 0;
    while (pic + 1 < n && doff[pic + 1] <= first) pic++;
    printf("blur PLANAR=%d DT=%d NC=%d shift=%u: %zu outputs, %u tiles, %s\n", (int)PLANAR, DT, NC, misalign_elems, n, work.form.blur_tiles, bad ? "MISMATCH" : "equal, guards intact");
    CHECK(bad == 0, "planar %d dtype %d channels %d shift %u: %zu bytes differ, the first at %zu (case %zu: %u x %u, %u taps, from %zu)", (int)PLANAR, DT, NC, misalign_elems, bad, first, pic,
          cs[pic].w, cs[pic].h, cs[pic].ksize, doff[pic]);
    free(src); free(dst); free(want); free(lds);
}

// ---- the resolver's rules for a blurred request --------------------------------------------------------------------------------------
static PjdResizeSpec small_spec(size_t n, bool views)
{
    PjdResizeSpec s;
    s.planar = true;
    for (size_t i = 0; i < n; i++) {
        s.pic.push_back(PjdResizePicture{i * 3000u, i * 4099u, 40, 25, 40});
        s.out_w.push_back(70); s.out_h.push_back(33);
        if (views) s.view_pic.push_back((uint32_t)(n - 1 - i));
    }
    return s;
}

static void resolver_rules()
{
    PjdResizeWork w;
    // the records, the shared rows and the identity flag
    {
        PjdResizeSpec s = small_spec(6, false);
        s.blur_set = true;
        s.blur = {pjd_blur{2.0, 23, 0}, pjd_blur{0.0, 0, 0}, pjd_blur{2.0, 23, 0}, pjd_blur{0.1, 3, 0}, pjd_blur{1.0, 1, 0}, pjd_blur{2.0, 5, 0}};
        const PjdResizeFault f = pjd_resize_resolve(s, w);
        CHECK(f.text.empty() && w.form.blurred && !w.form.padded && !w.form.windowed && !w.form.warp, "a blurred request keeps its resample's form: %s", f.text.c_str());
        CHECK(w.blur_taps.size() == 1 + 23 + 5 && w.blur_taps[0] == 65536, "row 0 and one row per distinct (ksize, sigma): %zu words", w.blur_taps.size());
        CHECK(w.blur[0].tap_off == 1 && w.blur[2].tap_off == 1 && w.blur[5].tap_off == 24 && w.blur[0].flags == 0 && w.blur[5].flags == 0, "equal pairs share one row");
        for (size_t i : {1u, 3u, 4u}) CHECK(w.blur[i].flags == PJD_BLUR_IDENTITY && w.blur[i].tap_off == 0, "output %zu is flagged the identity", i);
        CHECK(w.blur[3].ksize == 3 && w.blur[1].ksize == 0 && w.blur[0].ksize == 23, "ksize stays as asked for");
        uint32_t sum = 0;
        for (int j = 0; j < 23; j++) { sum += w.blur_taps[1 + j]; CHECK(w.blur_taps[1 + j] == w.blur_taps[1 + 22 - j], "symmetric"); }
        CHECK(sum == 65536, "the taps sum to 65536");
        const uint32_t per = ((70 + PJD_BLUR_COLS - 1) / PJD_BLUR_COLS) * ((33 + PJD_BLUR_ROWS - 1) / PJD_BLUR_ROWS);
        CHECK(w.form.blur_tiles == 6 * per && w.blur_prefix[3] == 3 * per && w.blur[2].col_tiles == 2 && w.blur[2].tw == 70 && w.blur[2].th == 33, "tiles of the blur launch");
        CHECK(w.form.blur_lds == pjd_blur_lds(11, 3), "LDS of the largest radius that is not an identity");
        const PjdPackedLayout lay = pjd_packed_layout(s.out_w.data(), s.out_h.data(), 6, 1, 3);
        CHECK(w.form.blur_buf_bytes == lay.buf_bytes, "the intermediate is the packed uint8 layout");
        for (size_t i = 0; i < 6; i++) CHECK(w.recs[i].dst_off == lay.off[i] && w.blur[i].src_off == lay.off[i] && w.blur[i].dst_off == i * 4099u && w.recs[i].src_off == i * 3000u, "offsets of output %zu", i);
        // a batch of identities: no halo at all
        s.blur.assign(6, pjd_blur{0.0, 0, 0});
        CHECK(pjd_resize_resolve(s, w).text.empty() && w.form.blurred && w.form.blur_lds == pjd_blur_lds(0, 3) && w.blur_taps.size() == 1, "an all-None request");
        // grey, affine and colour beside it
        s.blur[0] = pjd_blur{3.0, 63, 0}; s.channels = 1;
        CHECK(pjd_resize_resolve(s, w).text.empty() && w.form.blurred && w.form.padded && w.form.blur_lds == pjd_blur_lds(31, 1), "a grey blurred request");
        s.channels = 3; s.affine_set = true; s.affine.assign(6, PjdAffine{{1, 0, 0, 0, 1, 0}});
        s.colour_set = true; s.colour.assign(6, PjdColour{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}});
        CHECK(pjd_resize_resolve(s, w).text.empty() && w.form.blurred && w.form.warp && w.form.coloured && w.recs[4].dst_off == w.blur[4].src_off, "behind the warp and the colour map");
    }
    // the pad refusal, the request grown in both orders
    for (int order = 0; order < 2; order++) {
        PjdResizeSpec s = small_spec(2, false);
        auto add_pad = [&] { s.pad_set = true; s.pad.assign(2, pjd_resize_pad{0, 0, 0, 0}); };
        auto add_blur = [&] { s.blur_set = true; s.blur.assign(2, pjd_blur{1.0, 3, 0}); };
        if (order == 0) { add_pad(); add_blur(); } else { add_blur(); add_pad(); }
        const PjdResizeFault f = pjd_resize_resolve(s, w);
        CHECK(!f.state && f.picture == -1 && f.text.find("set_resize_pad") != std::string::npos && f.text.find("exclude") != std::string::npos, "pad order %d: %s", order, f.text.c_str());
    }
    // the fault texts, with and without views
    for (int views = 0; views < 2; views++) {
        PjdResizeSpec s = small_spec(3, views != 0);
        s.blur_set = true;
        const struct { pjd_blur e; const char *text; } bad[] = {
            {{1.0, 4, 0}, "ksize must be odd"}, {{1.0, 65, 0}, "ksize is beyond PJD_BLUR_MAX_TAPS"}, {{0.0, 3, 0}, "sigma must be finite and greater than 0"},
            {{-1.0, 3, 0}, "sigma must be finite and greater than 0"}, {{NAN, 3, 0}, "sigma must be finite and greater than 0"}, {{INFINITY, 3, 0}, "sigma must be finite and greater than 0"},
            {{0.5, 0, 0}, "sigma must be 0 where ksize == 0 (no blur)"}, {{1.0, 3, 1}, "reserved_ must be 0"}, {{0.0, 0, 7}, "reserved_ must be 0"}};
        for (const auto &b : bad) {
            s.blur.assign(3, pjd_blur{1.0, 3, 0});
            s.blur[1] = b.e;
            const PjdResizeFault f = pjd_resize_resolve(s, w);
            CHECK(!f.state && f.picture == 1 && f.text == std::string(views ? "view 1 (picture 1)" : "picture 1") + ": " + b.text, "text: %s", f.text.c_str());
            CHECK(pjd_blur_fault(&b.e) && std::string(pjd_blur_fault(&b.e)) == b.text, "pjd_blur_fault agrees");
        }
        s.blur.assign(3, pjd_blur{5e-324, 63, 0});
        CHECK(pjd_resize_resolve(s, w).text.empty() && w.blur[0].flags == PJD_BLUR_IDENTITY, "the smallest sigma is the identity");
        s.blur.assign(3, pjd_blur{1e308, 63, 0});
        CHECK(pjd_resize_resolve(s, w).text.empty() && w.blur[0].flags == 0 && w.blur_taps.size() == 64, "the largest sigma is a box");
    }
    CHECK(pjd_blur_fault(nullptr) != nullptr, "null");
    // a request without the call resolves to what it did
    PjdResizeSpec plain = small_spec(2, false);
    CHECK(pjd_resize_resolve(plain, w).text.empty() && !w.form.blurred && w.blur.empty() && w.blur_taps.empty() && w.form.blur_tiles == 0 && w.form.blur_buf_bytes == 0 && w.recs[1].dst_off == 4099,
          "a request without a blur is untouched");
    // the border rule against repeated reflection
    for (uint32_t n : {1u, 2u, 3u, 7u, 64u, 65535u})
        for (int32_t i = -200; i <= 200; i++) CHECK(pjd_blur_index_calc(n, i) == reflect(n, i) && pjd_blur_index_calc(n, (int32_t)n - 1 + i) == reflect(n, (int64_t)n - 1 + i), "index %d of %u", i, n);
    printf("blurred request: resolver rules checked\n");
}

int main(int argc, char **argv)
{
    resolver_rules();
    run<true, 0, 3>(0, 1, argc > 1 ? argv[1] : nullptr);
    run<false, 0, 3>(1, 2, nullptr);
    run<true, 0, 1>(3, 3, nullptr);
    for (uint32_t mis = 0; mis < 4; mis++) {
        run<false, PJD_DT_F16, 3>(mis, 21 + mis, nullptr); run<false, PJD_DT_BF16, 3>(mis, 31 + mis, nullptr); run<false, PJD_DT_F32, 3>(mis, 41 + mis, nullptr);
        run<true, PJD_DT_F16, 3>(mis, 61 + mis, nullptr);  run<true, PJD_DT_BF16, 3>(mis, 71 + mis, nullptr);  run<true, PJD_DT_F32, 3>(mis, 81 + mis, nullptr);
        run<true, PJD_DT_F16, 1>(mis, 101 + mis, nullptr); run<true, PJD_DT_BF16, 1>(mis, 111 + mis, nullptr); run<true, PJD_DT_F32, 1>(mis, 121 + mis, nullptr);
    }
    printf("%s, %d checks failed; no sanitizer report\n", failed ? "DIFFERENCES" : "ALL EQUAL", failed);
    return failed ? 1 : 0;
}
