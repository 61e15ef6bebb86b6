// resize_body_host.cpp -- the body of the resample kernels (pim-jpeg-decoder_amd/csrc/pjd_k_resize_body.h) run on the host, thread by
// thread, under the sanitizers: indexing, tile search, the vector and the element store paths at every alignment, guard bytes.
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize=alignment -Wno-builtin-macro-redefined -Wno-keyword-macro \
//         -o resize_body_host tools/resize_body_host.cpp && ./resize_body_host
//
// The device builtins are replaced by host stand-ins (a lane's row taps are computed directly instead of being read from lane k; the
// 16-bit conversions are bit functions), so this says nothing about what the GPU's conversions do -- tests/test_gpu_normalize.py does.
// Every variant (uint8 / fp16 / bf16 / fp32, planar / interleaved) writes 31 pictures (tile edges, ragged right edges, random sizes)
// into one buffer at element-aligned offsets with odd gaps, the buffer itself shifted by 0..3 elements; the result is compared byte for
// byte with a plain per-pixel loop over the arithmetic of include/pjd.h, bytes between the pictures included.  Prints ALL EQUAL.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
#define __restrict__
#include "../include/pjd.h"
#include "../pim-jpeg-decoder_amd/csrc/pjd_internal.h"
struct Dim { uint32_t x; };
static thread_local Dim threadIdx, blockIdx;
static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xffffff) * (b & 0xffffff); }
static inline uint32_t lerp8(uint32_t a, uint32_t b, uint32_t w) { return __umul24(256u - w, a) + __umul24(w, b); }
struct NormArgs { float scale[3], bias[3]; };
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
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
// stand-ins for the device types: conversion = the bit functions above
struct H16 { uint16_t b; H16() {} explicit H16(float f) : b(f16bits(f)) {} };
struct B16 { uint16_t b; B16() {} explicit B16(float f) : b(bf16bits(f)) {} };
#define _Float16 H16
#define __bf16 B16
template <int DT> static inline uint32_t norm_pair16(uint32_t v0, uint32_t v1, float scale, float bias)
{
    const float a = pjd_normalize_f32(v0, scale, bias), b = pjd_normalize_f32(v1, scale, bias);
    if (DT == PJD_DT_F16) return f16bits(a) | ((uint32_t)f16bits(b) << 16);
    return bf16bits(a) | ((uint32_t)bf16bits(b) << 16);
}
template <class T, class F> static inline T my_bit_cast(F f) { T t; static_assert(sizeof(T) == sizeof(F), ""); memcpy(&t, &f, sizeof t); return t; }
#define __builtin_bit_cast(T, v) my_bit_cast<T>(v)
#define __builtin_amdgcn_readfirstlane(x) (x)
static inline uint32_t emu_tap(uint32_t sh, uint32_t th, uint32_t row) { uint32_t y0, y1, wy; pjd_resize_tap_calc(sh, th, row < th ? row : th - 1, y0, y1, wy); return y0 | (wy << 16); }
#define __builtin_amdgcn_readlane(p, k) emu_tap(r.sh, r.th, row0 + (k))

template <bool PLANAR, int DT>
static void thread_body(const uint8_t *src, uint8_t *dst, const PjdDevResize *recs, const uint32_t *tile_prefix, uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
#include "../pim-jpeg-decoder_amd/csrc/pjd_k_resize_body.h"
}

template <bool PLANAR, int DT>
static int run(uint32_t misalign_elems, unsigned seed)
{
    const uint32_t ES = DT == 0 ? 1 : PJD_DT_SIZE(DT);
    struct Case { uint32_t sw, sh, tw, th; };
    std::vector<Case> cases = {{61,45,1,1},{61,45,5,9},{88,56,256,8},{88,56,257,9},{80,96,259,3},{33,70,7,17},{61,45,61,45},{88,56,88,56},{17,9,300,2},{1,1,9,9},{300,1,3,5}};
    srand(seed);
    for (int k = 0; k < 20; k++) cases.push_back({(uint32_t)(1 + rand() % 120), (uint32_t)(1 + rand() % 120), (uint32_t)(1 + rand() % 300), (uint32_t)(1 + rand() % 300)});
    const size_t n = cases.size();
    std::vector<PjdDevResize> recs(n); std::vector<uint32_t> prefix(n + 1);
    size_t spos = 0, dpos = misalign_elems * ES; uint32_t t = 0;
    std::vector<size_t> doff(n), dbytes(n);
    for (size_t i = 0; i < n; i++) {
        auto &c = cases[i]; PjdDevResize &r = recs[i];
        r.src_off = spos; r.sw = c.sw; r.sh = c.sh; r.src_stride = PLANAR ? c.sw : 3 * c.sw; r.tw = c.tw; r.th = c.th;
        r.col_tiles = (c.tw + PJD_RS_COLS - 1) / PJD_RS_COLS; r.dst_off = dpos;
        doff[i] = dpos; dbytes[i] = 3ull * c.tw * c.th * ES;
        spos += 3ull * c.sw * c.sh; dpos += dbytes[i] + ES * (2 * (i % 3) + 1);      // element-aligned odd gaps
        prefix[i] = t; t += r.col_tiles * ((c.th + PJD_RS_ROWS - 1) / PJD_RS_ROWS);
    }
    prefix[n] = t;
    std::vector<uint8_t> src(spos); for (auto &b : src) b = (uint8_t)rand();
    uint8_t *dst = (uint8_t *)aligned_alloc(256, (dpos + 511) & ~255ull); memset(dst, 0xA5, dpos + 256);
    NormArgs nz = {{0.01712475f, 0.017507f, -0.01742919f}, {-2.117904f, -2.0357144f, 1.8044444f}};
    const uint32_t n_blocks = (t + PJD_RS_WAVES - 1) / PJD_RS_WAVES;
    for (uint32_t b = 0; b < n_blocks; b++) for (uint32_t th = 0; th < 64 * PJD_RS_WAVES; th++) { blockIdx.x = b; threadIdx.x = th; thread_body<PLANAR, DT>(src.data(), dst, recs.data(), prefix.data(), (uint32_t)n, t, nz); }
    // reference
    std::vector<uint8_t> want(dpos + 256, 0xA5);
    for (size_t i = 0; i < n; i++) {
        auto &c = cases[i]; const uint8_t *sp = src.data() + recs[i].src_off;
        for (uint32_t y = 0; y < c.th; y++) for (uint32_t x = 0; x < c.tw; x++) for (int ch = 0; ch < 3; ch++) {
            uint32_t x0, x1, wx, y0, y1, wy;
            pjd_resize_tap_calc(c.sw, c.tw, x, x0, x1, wx); pjd_resize_tap_calc(c.sh, c.th, y, y0, y1, wy);
            auto P = [&](uint32_t yy, uint32_t xx) -> uint32_t { return PLANAR ? sp[(size_t)ch * c.sw * c.sh + (size_t)yy * c.sw + xx] : sp[((size_t)yy * c.sw + xx) * 3 + ch]; };
            const uint32_t v = ((256 - wy) * ((256 - wx) * P(y0, x0) + wx * P(y0, x1)) + wy * ((256 - wx) * P(y1, x0) + wx * P(y1, x1)) + 32768) >> 16;
            const size_t e = PLANAR ? ((size_t)ch * c.th + y) * c.tw + x : ((size_t)y * c.tw + x) * 3 + ch;
            uint8_t *o = want.data() + doff[i] + e * ES;
            if (DT == 0) *o = (uint8_t)v;
            else {
                const float u = fmaf((float)v, nz.scale[ch], nz.bias[ch]);
                if (DT == PJD_DT_F32) memcpy(o, &u, 4);
                else { const uint16_t h = DT == PJD_DT_F16 ? f16bits(u) : bf16bits(u); memcpy(o, &h, 2); }
            }
        }
    }
    int bad = 0;
    for (size_t k = 0; k < dpos + 256; k++) if (dst[k] != want[k]) { if (bad < 4) printf("  mismatch at byte %zu got %02x want %02x\n", k, dst[k], want[k]); bad++; }
    printf("PLANAR=%d DT=%d misalign=%u: %zu pictures, %u tiles, %zu bytes: %s\n", (int)PLANAR, DT, misalign_elems, n, t, dpos, bad ? "MISMATCH" : "equal, guards intact");
    free(dst);
    return bad != 0;
}

int main()
{
    int rc = 0;
    for (uint32_t mis : {0u, 1u, 2u, 3u}) {
        rc |= run<true, 0>(mis, 1); rc |= run<false, 0>(mis, 2);
        rc |= run<true, PJD_DT_F16>(mis, 3); rc |= run<false, PJD_DT_F16>(mis, 4);
        rc |= run<true, PJD_DT_BF16>(mis, 5); rc |= run<false, PJD_DT_BF16>(mis, 6);
        rc |= run<true, PJD_DT_F32>(mis, 7); rc |= run<false, PJD_DT_F32>(mis, 8);
    }
    printf(rc ? "FAILED\n" : "ALL EQUAL\n");
    return rc;
}
