// resize_plan_host.cpp -- the resolver of the resample work list (pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp) on the CPU, under the
// sanitizers: every limit on both sides of its boundary with the picture it names, a seeded family over the full cross of pads,
// orientations, windows, filters and layouts whose records are held against statements written out HERE from include/pjd.h (never
// against the helpers under test), and the setters' order: the request built up call by call resolves to what it resolves to in one go;
// and the rules of a colour map (pjd_batch_set_colour): limits, records, the identity flag, the padded form it brings.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__host__= -D__device__= -o resize_plan_host
//         tools/resize_plan_host.cpp pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp && ./resize_plan_host
//
// tests/test_resize_plan_cpu.py builds and runs it.  Prints `no sanitizer report` at the end; exit status 1 where a check failed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../pim-jpeg-decoder_amd/csrc/pjd_resize_plan.h"

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_bad++ < 20) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t g_seed = 1;
static uint32_t rnd(uint32_t n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }   // 0 .. n-1

// a request of n pictures sw x sh -> tw x th, sources and results back to back
static PjdResizeSpec plain_spec(size_t n, uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, bool planar = false)
{
    PjdResizeSpec s;
    s.planar = planar;
    for (size_t i = 0; i < n; i++) {
        s.pic.push_back(PjdResizePicture{i * 3ull * sw * sh, i * 3ull * tw * th, sw, sh, planar ? sw : 3 * sw});
        s.out_w.push_back(tw); s.out_h.push_back(th);
    }
    return s;
}

// picture -2: the request resolves; else: it is refused, and the fault names this picture (-1: the batch)
static void expect(const PjdResizeSpec &s, int picture, const char *what)
{
    PjdResizeWork w;
    const PjdResizeFault f = pjd_resize_resolve(s, w);
    if (picture == -2) CHECK(f.text.empty(), "%s: refused: %s", what, f.text.c_str());
    else {
        CHECK(!f.text.empty() && f.picture == picture, "%s: %s, picture %d (expected %d)", what, f.text.empty() ? "accepted" : f.text.c_str(), f.picture, picture);
        if (picture >= 0) CHECK(f.text.find("picture " + std::to_string(picture)) != std::string::npos, "%s: the text does not name the picture: %s", what, f.text.c_str());
    }
}

static PjdResizeSpec with_window(PjdResizeSpec s, size_t i, pjd_resize_window w)
{
    s.win_set = true; s.win.assign(s.pic.size(), pjd_resize_window{});
    s.win[i] = w;
    return s;
}
static PjdResizeSpec with_pad(PjdResizeSpec s, size_t i, pjd_resize_pad p)
{
    s.pad_set = true; s.pad.assign(s.pic.size(), pjd_resize_pad{});
    s.pad[i] = p;
    return s;
}
static PjdResizeSpec with_filter(PjdResizeSpec s, int filter) { s.filter_set = true; s.filter = filter; return s; }

static void limits()
{
    const uint32_t M = 0xffffffffu;
    // ---- targets: 0 | 1 .. 65535 | 65536
    for (int axis = 0; axis < 2; axis++)
        for (uint32_t v : {0u, 1u, 65535u, 65536u}) {
            PjdResizeSpec s = plain_spec(3, 40, 30, 20, 10);
            (axis ? s.out_h : s.out_w)[2] = v;
            expect(s, v == 0 || v == 65536u ? 2 : -2, "target size");
        }
    // ---- orientations: 0 | 1 .. 8 | 9
    for (uint32_t o : {0u, 1u, 8u, 9u}) {
        PjdResizeSpec s = plain_spec(3, 40, 30, 20, 10);
        s.ori_set = true; s.orientation = {1, (uint8_t)o, 1};
        expect(s, o == 0 || o == 9 ? 1 : -2, "orientation");
    }
    // ---- windows, clause by clause; the picture is 40 x 30, its target 20 x 10
    const PjdResizeSpec base = plain_spec(3, 40, 30, 20, 10);
    struct W { pjd_resize_window w; bool ok; const char *what; };
    const W wins[] = {
        {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, true, "all defaults"},
        {{0, 0, 0, 5, 0, 0, 0, 0, 0, 0}, false, "w == 0, h != 0"}, {{0, 0, 5, 0, 0, 0, 0, 0, 0, 0}, false, "h == 0, w != 0"},
        {{1, 0, 0, 0, 0, 0, 0, 0, 0, 0}, false, "x without a window"}, {{0, 1, 0, 0, 0, 0, 0, 0, 0, 0}, false, "y without a window"},
        {{35, 0, 5, 30, 0, 0, 0, 0, 0, 0}, true, "x + w == sw"}, {{36, 0, 5, 30, 0, 0, 0, 0, 0, 0}, false, "x + w == sw + 1"}, {{M, 0, 2, 30, 0, 0, 0, 0, 0, 0}, false, "x + w wraps"},
        {{0, 25, 40, 5, 0, 0, 0, 0, 0, 0}, true, "y + h == sh"}, {{0, 26, 40, 5, 0, 0, 0, 0, 0, 0}, false, "y + h == sh + 1"}, {{0, M, 40, 2, 0, 0, 0, 0, 0, 0}, false, "y + h wraps"},
        {{0, 0, 0, 0, 65535, 0, 0, 0, 0, 0}, true, "vw == 65535"}, {{0, 0, 0, 0, 65536, 0, 0, 0, 0, 0}, false, "vw == 65536"},
        {{0, 0, 0, 0, 0, 65535, 0, 0, 0, 0}, true, "vh == 65535"}, {{0, 0, 0, 0, 0, 65536, 0, 0, 0, 0}, false, "vh == 65536"},
        {{0, 0, 0, 0, 25, 0, 5, 0, 0, 0}, true, "ox + tw == vw"}, {{0, 0, 0, 0, 25, 0, 6, 0, 0, 0}, false, "ox + tw == vw + 1"}, {{0, 0, 0, 0, 25, 0, M, 0, 0, 0}, false, "ox + tw wraps"},
        {{0, 0, 0, 0, 0, 0, 1, 0, 0, 0}, false, "ox against the default vw"},
        {{0, 0, 0, 0, 0, 13, 0, 3, 0, 0}, true, "oy + th == vh"}, {{0, 0, 0, 0, 0, 13, 0, 4, 0, 0}, false, "oy + th == vh + 1"}, {{0, 0, 0, 0, 0, 13, 0, M, 0, 0}, false, "oy + th wraps"},
        {{0, 0, 0, 0, 0, 0, 0, 0, PJD_RW_HFLIP, 0}, true, "the flip"}, {{0, 0, 0, 0, 0, 0, 0, 0, 2, 0}, false, "an unknown flag"}, {{0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, false, "reserved_"}};
    for (const W &c : wins) expect(with_window(base, 1, c.w), c.ok ? -2 : 1, c.what);
    for (uint32_t sw : {0u, 65535u, 65536u}) {              // the decode size the window is held against
        PjdResizeSpec s = with_window(base, 2, pjd_resize_window{});
        s.pic[2].sw = sw;
        expect(s, sw == 65535u ? -2 : 2, "decode width under a window");
    }
    // ... against Q's target: orientation 6 swaps it to 10 x 20, a pad shrinks it first
    {
        PjdResizeSpec s = with_window(base, 1, {0, 0, 0, 0, 15, 0, 5, 0, 0, 0});
        expect(s, 1, "ox + tw against the unswapped target");
        s.ori_set = true; s.orientation = {1, 6, 1};
        expect(s, -2, "ox + tw against the swapped target");
        expect(with_pad(with_window(base, 1, {0, 0, 0, 0, 15, 0, 5, 0, 0, 0}), 1, {6, 0, 4, 0}), -2, "ox + tw against the content");
    }
    // ---- pads: the canvas is 20 x 10
    struct P { pjd_resize_pad p; bool ok; const char *what; };
    const P pads[] = {{{10, 0, 9, 0}, true, "left + right == out_w - 1"}, {{10, 0, 10, 0}, false, "left + right == out_w"}, {{M, 0, 2, 0}, false, "left + right wraps"},
                      {{0, 4, 0, 5}, true, "top + bottom == out_h - 1"}, {{0, 5, 0, 5}, false, "top + bottom == out_h"}, {{0, 1u << 31, 0, 1u << 31}, false, "top + bottom wraps"}};
    for (const P &c : pads) expect(with_pad(base, 2, c.p), c.ok ? -2 : 2, c.what);
    // ---- 16x an axis: the table-driven filters refuse 16x + 1, the bilinear one takes it; the limit is the window's where there is one
    for (int filter : {PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC})
        for (int axis = 0; axis < 2; axis++)
            for (uint32_t over : {0u, 1u}) {
                const int want = over && filter != PJD_RESIZE_BILINEAR ? 1 : -2;
                PjdResizeSpec s = plain_spec(3, 40, 30, 20, 10);
                s.pic[1] = axis ? PjdResizePicture{0, 0, 40, 160 + over, 120} : PjdResizePicture{0, 0, 320 + over, 30, 3 * (320 + over)};
                expect(with_filter(s, filter), want, "16x, plain");
                // a 200 x 200 picture to 3 x 3 (far more than 16x) through a window of 80 or 81 samples to a virtual target of 5
                s = plain_spec(3, 200, 200, 3, 3);
                const uint32_t len = 80 + over;
                s = with_window(s, 1, axis ? pjd_resize_window{0, 7, 48, len, 0, 5, 0, 1, 0, 0} : pjd_resize_window{7, 0, len, 48, 5, 0, 1, 0, 0, 0});
                for (size_t i : {0, 2}) s.win[i] = {0, 0, 16, 16, 0, 0, 0, 0, 0, 0};
                expect(with_filter(s, filter), want, "16x, windowed");
            }
    // ---- the longest axes: 65535 samples to 65535 and to 4096 (16x: 65536), one row and one column
    for (int filter : {PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC})
        for (int axis = 0; axis < 2; axis++)
            for (uint32_t dn : {65535u, 4096u, 4095u}) {
                PjdResizeSpec s = axis ? plain_spec(2, 1, 65535, 1, dn, true) : plain_spec(2, 65535, 1, dn, 1);
                PjdResizeWork w;
                const PjdResizeFault f = pjd_resize_resolve(with_filter(s, filter), w);
                if (dn == 4095u) CHECK(f.picture == 0, "65535 -> 4095 is more than 16x: %s", f.text.c_str());
                else CHECK(f.text.empty() && w.form.tiles == 2 * (axis ? (dn + 7) / 8 : (dn + 255) / 256) && w.aa[0].x_tab == w.aa[1].x_tab && w.aa[0].y_tab == w.aa[1].y_tab, "65535 -> %u: %s", dn, f.text.c_str());
            }
    // ---- one launch: tiles and border lines below 2^31.  65535 x 65535 is 256 x 8192 = 2^21 tiles
    expect(plain_spec(1023, 8, 8, 65535, 65535), -2, "1023 x 2^21 tiles");
    expect(plain_spec(1024, 8, 8, 65535, 65535), -1, "1024 x 2^21 tiles");
    for (int planar = 0; planar < 2; planar++) {
        // canvases 2 x 65535 with one column of pad: 65535 lines each, three times that planar
        const size_t most = planar ? 10922 : 32768;             // 10922 * 3 * 65535 < 2^31 <= 10923 * 3 * 65535; 32768 * 65535 < 2^31 <= 32769 * 65535
        for (size_t n : {most, most + 1}) {
            PjdResizeSpec s = plain_spec(n, 8, 8, 2, 65535, planar != 0);
            s.pad_set = true; s.pad.assign(n, pjd_resize_pad{1, 0, 0, 0});
            expect(s, n == most ? -2 : -1, "border lines");
            s.pad.assign(n, pjd_resize_pad{});                   // all zero: no border line at all
            expect(s, -2, "border lines of an all-zero pad");
        }
    }
    expect(with_filter(base, 2), -1, "an unknown filter");
}

// ---- the statements of include/pjd.h, written out ---------------------------------------------------------------------------------------
// the bits t << 2 | v << 1 | h of an orientation 1..8: D = H^h(V^v(T^t(Q)))
static uint32_t tvh_of(uint32_t o) { return o == 1 ? 0u : o == 2 ? 1u : o == 3 ? 3u : o == 4 ? 2u : o == 5 ? 4u : o == 6 ? 5u : o == 7 ? 7u : 6u; }
// ... and what the kernels do for it: bit 0 mirrors the column tap index, bit 1 the position a row of Q is stored at, bit 2 stores Q's
// columns as D's rows.  t = 0: tap mirror h, store mirror v; t = 1: tap mirror v, store mirror h
static uint32_t flags_of(uint32_t o)
{
    const uint32_t b = tvh_of(o), t = b >> 2, v = (b >> 1) & 1u, h = b & 1u;
    return t ? 4u | (v ? 1u : 0u) | (h ? 2u : 0u) : (h ? 1u : 0u) | (v ? 2u : 0u);
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T))); }
static bool same(const PjdResizeWork &a, const PjdResizeWork &b)
{
    return a.form.tiles == b.form.tiles && a.form.lines == b.form.lines && a.form.lds == b.form.lds && a.form.windowed == b.form.windowed && a.form.oriented == b.form.oriented &&
           a.form.padded == b.form.padded && same(a.recs, b.recs) && same(a.tile_prefix, b.tile_prefix) && same(a.win, b.win) && same(a.pad, b.pad) && same(a.line_prefix, b.line_prefix) &&
           same(a.aa, b.aa) && same(a.tab, b.tab) && same(a.ct_w, b.ct_w) && same(a.ct_h, b.ct_h);
}

// one member of the family.  pads / oris / wins: 0 absent, 1 present and neutral, 2 mixed
static void family(int pads, int oris, int wins, int filter, bool planar, uint32_t seed)
{
    g_seed = seed;
    const size_t n = 6;
    const bool table = filter != PJD_RESIZE_BILINEAR;
    PjdResizeSpec s;
    s.planar = planar;
    std::vector<uint32_t> qw(n), qh(n);                         // Q's target, by the statement: the canvas less its pad, swapped for 5..8
    uint64_t spos = 0, dpos = 5;
    for (size_t i = 0; i < n; i++) {
        // picture 1 crosses a column tile (the canvas is at least 280 wide), picture 2 has neither pad nor orientation nor window
        const uint32_t W = i == 1 ? 280 + rnd(21) : 1 + rnd(300), H = 1 + rnd(i == 1 ? 12 : 300);
        pjd_resize_pad p{};
        if (pads == 2 && i != 2) { p.left = rnd(std::min(W, 9u)); p.right = rnd(std::min(W - p.left, 9u)); p.top = rnd(std::min(H, 9u)); p.bottom = rnd(std::min(H - p.top, 9u)); }
        if (pads == 2 && i == 1) p.left = 1 + rnd(8);           // ... and picture 1 has one for certain
        const uint32_t o = oris == 2 && i != 2 ? (i == 0 ? 6u : 1 + rnd(8)) : 1u;
        const uint32_t cw = W - p.left - p.right, ch = H - p.top - p.bottom;
        qw[i] = o >= 5 ? ch : cw; qh[i] = o >= 5 ? cw : ch;
        // a source the table-driven filters take without a window: at most 16x Q's target
        const uint32_t sw = 1 + rnd(std::min(300u, 16 * qw[i])), sh = 1 + rnd(std::min(300u, 16 * qh[i]));
        pjd_resize_window w{};
        if (wins == 2 && i != 2 && i != 4) {                    // picture 4: a record of zeros among the others
            w.w = 1 + rnd(sw); w.h = 1 + rnd(sh); w.x = rnd(sw - w.w + 1); w.y = rnd(sh - w.h + 1);
            w.ox = rnd(5); w.oy = rnd(5);
            w.vw = i == 3 ? 0 : qw[i] + w.ox + rnd(7);          // picture 3: the default virtual target, so no offset
            w.vh = i == 3 ? 0 : qh[i] + w.oy + rnd(7);
            if (i == 3) w.ox = w.oy = 0;
            w.flags = i == 0 ? PJD_RW_HFLIP : rnd(2);
        }
        s.pic.push_back(PjdResizePicture{spos, dpos, sw, sh, planar ? sw : 3 * sw});
        s.out_w.push_back(W); s.out_h.push_back(H);
        s.pad.push_back(p); s.orientation.push_back((uint8_t)o); s.win.push_back(w);
        spos += 3ull * sw * sh; dpos += 3ull * W * H + 2 * i + 1;
    }
    s.pad_set = pads != 0; s.ori_set = oris != 0; s.win_set = wins != 0; s.filter_set = true; s.filter = filter;
    if (!pads) s.pad.clear();
    if (!oris) s.orientation.clear();
    if (!wins) s.win.clear();
    char what[96];
    snprintf(what, sizeof what, "pads %d oris %d wins %d filter %d planar %d", pads, oris, wins, filter, (int)planar);

    PjdResizeWork k;
    const PjdResizeFault f = pjd_resize_resolve(s, k);
    CHECK(f.text.empty(), "%s: refused: %s", what, f.text.c_str());
    if (!f.text.empty()) return;

    // the form: a neutral array changes nothing, not one byte of one record
    const bool padded = pads == 2, oriented = padded || oris == 2, windowed = oriented || wins == 2;
    CHECK(k.form.padded == padded && k.form.oriented == oriented && k.form.windowed == windowed, "%s: form %d %d %d", what, k.form.windowed, k.form.oriented, k.form.padded);
    CHECK(k.win.size() == (windowed ? n : 0) && k.pad.size() == (padded ? n : 0) && k.line_prefix.size() == (padded ? n + 1 : 0) && k.aa.size() == (table ? n : 0) && k.tab.empty() == !table, "%s: records the form does not read", what);
    if (pads == 1 || oris == 1 || wins == 1) {
        PjdResizeSpec a = s;
        if (pads == 1) { a.pad_set = false; a.pad.clear(); }
        if (oris == 1) { a.ori_set = false; a.orientation.clear(); }
        if (wins == 1) { a.win_set = false; a.win.clear(); }
        PjdResizeWork ka;
        CHECK(pjd_resize_resolve(a, ka).text.empty() && same(k, ka), "%s: a neutral array changed the records", what);
    }
    uint32_t tiles = 0, lines = 0;
    CHECK(k.recs.size() == n && k.tile_prefix.size() == n + 1 && k.ct_w.size() == n && k.ct_h.size() == n, "%s: sizes", what);
    for (size_t i = 0; i < n; i++) {
        const PjdDevResize &r = k.recs[i];
        const pjd_resize_pad p = pads ? s.pad[i] : pjd_resize_pad{};
        const uint32_t o = oris ? s.orientation[i] : 1u;
        const pjd_resize_window w = wins ? s.win[i] : pjd_resize_window{};
        // content = canvas - pad; Q's target swapped exactly for 5..8; the rest as the caller gave it
        CHECK(k.ct_w[i] == s.out_w[i] - p.left - p.right && k.ct_h[i] == s.out_h[i] - p.top - p.bottom, "%s: content of picture %zu", what, i);
        CHECK(r.tw == (o >= 5 ? k.ct_h[i] : k.ct_w[i]) && r.th == (o >= 5 ? k.ct_w[i] : k.ct_h[i]) && r.tw == qw[i] && r.th == qh[i], "%s: Q's target of picture %zu", what, i);
        CHECK(r.src_off == s.pic[i].src_off && r.dst_off == s.pic[i].dst_off && r.sw == s.pic[i].sw && r.sh == s.pic[i].sh && r.src_stride == s.pic[i].src_stride, "%s: picture %zu as given", what, i);
        CHECK(r.col_tiles == (r.tw + 255) / 256 && k.tile_prefix[i] == tiles, "%s: tiles of picture %zu", what, i);
        tiles += ((r.tw + 255) / 256) * ((r.th + 7) / 8);
        // the window: defaults against the decode size and Q's target; the flip XOR the orientation's bits
        const PjdDevResizeWin want{w.x, w.y, w.w ? w.w : r.sw, w.h ? w.h : r.sh, w.vw ? w.vw : qw[i], w.vh ? w.vh : qh[i], w.ox, w.oy, w.flags ^ flags_of(o), 0u};
        if (windowed) CHECK(!memcmp(&k.win[i], &want, sizeof want), "%s: window of picture %zu", what, i);
        if (padded) {
            const PjdDevResizePad &c = k.pad[i];
            CHECK(c.W == s.out_w[i] && c.H == s.out_h[i] && c.left == p.left && c.top == p.top && c.cw == k.ct_w[i] && c.ch == k.ct_h[i] && k.line_prefix[i] == lines, "%s: canvas of picture %zu", what, i);
            if (p.left || p.top || p.right || p.bottom) lines += (planar ? 3u : 1u) * s.out_h[i];
        }
        if (!table) continue;
        // the tables: every head inside its axis, every sample's weights sum to 1, and the LDS holds the span of every tile
        const PjdDevResizeAA &a = k.aa[i];
        const uint32_t *x = k.tab.data() + a.x_tab, *y = k.tab.data() + a.y_tab;
        for (int axis = 0; axis < 2; axis++) {
            const uint32_t *t = axis ? y : x, sn = axis ? want.h : want.w, dn = axis ? want.vh : want.vw, taps = axis ? a.y_taps : a.x_taps;
            CHECK((size_t)(t - k.tab.data()) + (size_t)dn * (1 + taps) <= k.tab.size() && taps >= 1 && taps <= (filter == PJD_RESIZE_BICUBIC ? 64u : 32u), "%s: table of picture %zu", what, i);
            for (uint32_t j = 0; j < dn; j++) {
                const uint32_t first = t[j] & 0xffffu, cnt = t[j] >> 16;
                int64_t sum = 0;
                for (uint32_t q = 0; q < taps; q++) {
                    const int64_t wq = filter == PJD_RESIZE_BICUBIC ? (int64_t)(int32_t)t[(size_t)(q + 1) * dn + j] : (int64_t)t[(size_t)(q + 1) * dn + j];
                    if (q >= cnt) CHECK(wq == 0, "%s: a weight behind the count", what);
                    sum += wq;
                }
                CHECK(cnt >= 1 && cnt <= taps && first + cnt <= sn && sum == 65536, "%s: picture %zu axis %d sample %u: first %u count %u of %u, sum %lld", what, i, axis, j, first, cnt, sn, (long long)sum);
            }
        }
        for (uint32_t c0 = 0; c0 < r.tw; c0 += 256) {
            uint32_t lo = ~0u, hi = 0;
            for (uint32_t c = c0; c < std::min(c0 + 256, r.tw); c++) {
                const uint32_t head = x[want.ox + ((want.flags & 1u) ? r.tw - 1 - c : c)];
                lo = std::min(lo, head & 0xffffu); hi = std::max(hi, (head & 0xffffu) + (head >> 16));
            }
            const uint32_t span = hi - lo, need = planar ? 3 * ((span + 6) & ~3u) : (3 * span + 6) & ~3u;
            CHECK(k.form.lds >= need, "%s: picture %zu tile column %u stages %u bytes, the launch has %u", what, i, c0, need, k.form.lds);
        }
    }
    CHECK(k.tile_prefix[n] == tiles && k.form.tiles == tiles, "%s: the tile prefix sum ends at %u, not %u", what, k.tile_prefix[n], tiles);
    if (padded) CHECK(k.line_prefix[n] == lines && k.form.lines == lines, "%s: the line prefix sum ends at %u, not %u", what, k.line_prefix[n], lines);
    else CHECK(k.form.lines == 0, "%s: border lines without a pad", what);
    if (!table) CHECK(k.form.lds == 0, "%s: LDS without a table", what);

    // the setters' order: the request grown call by call -- pad, orientation, window, filter -- resolves at every step, and at the
    // last one to what the whole request resolves to in one go
    PjdResizeSpec g;
    g.pic = s.pic; g.planar = s.planar; g.out_w = s.out_w; g.out_h = s.out_h;
    PjdResizeWork kg;
    bool ok = pjd_resize_resolve(g, kg).text.empty();
    if (pads) { g.pad_set = true; g.pad = s.pad; ok = ok && pjd_resize_resolve(g, kg).text.empty(); }
    if (oris) { g.ori_set = true; g.orientation = s.orientation; ok = ok && pjd_resize_resolve(g, kg).text.empty(); }
    if (wins) { g.win_set = true; g.win = s.win; ok = ok && pjd_resize_resolve(g, kg).text.empty(); }
    CHECK(ok && kg.tab.empty() && kg.form.lds == 0 && same(kg.recs, k.recs) && same(kg.win, k.win) && same(kg.pad, k.pad), "%s: the request without its filter", what);
    g.filter_set = true; g.filter = filter;
    CHECK(pjd_resize_resolve(g, kg).text.empty() && same(kg, k), "%s: call by call is not in one go", what);
}

// the packed layout and the fill pattern, against their statements
static void layout_and_fill()
{
    const uint32_t w[3] = {5, 256, 1}, h[3] = {3, 1, 1};
    for (uint64_t es : {1, 2, 4}) {
        const PjdPackedLayout l = pjd_packed_layout(w, h, 3, es);
        CHECK(l.off[0] == 0 && l.off[1] == 256 && l.off[2] == 256 + ((768 * es + 255) & ~255ull) && l.bytes[0] == 45 * es && l.bytes[1] == 768 * es && l.bytes[2] == 3 * es &&
              l.sum == 816 * es && l.buf_bytes == l.off[2] + 256, "the packed layout at element size %llu", (unsigned long long)es);
    }
    const uint8_t fill[3] = {114, 7, 201};
    PjdNormalize nz{0, {1.0f, 0.5f, 2.0f}, {0.0f, 1.0f, -1.0f}};
    PjdPadFill f = pjd_pad_fill(nz, false, fill, nullptr);
    CHECK(f.d[0] == 0x72c90772u && f.d[1] == 0x0772c907u && f.d[2] == 0xc90772c9u, "uint8, interleaved: %08x %08x %08x", f.d[0], f.d[1], f.d[2]);
    f = pjd_pad_fill(nz, true, fill, nullptr);
    CHECK(f.d[0] == 0x72727272u && f.d[1] == 0x07070707u && f.d[2] == 0xc9c9c9c9u, "uint8, planar");
    nz.dtype = PJD_DT_F32;                                       // 114, 4.5, 401: exact in every type
    f = pjd_pad_fill(nz, false, fill, nullptr);
    CHECK(f.d[0] == 0x42e40000u && f.d[1] == 0x40900000u && f.d[2] == 0x43c88000u, "binary32: %08x %08x %08x", f.d[0], f.d[1], f.d[2]);
    nz.dtype = PJD_DT_BF16;
    f = pjd_pad_fill(nz, false, fill, nullptr);
    CHECK(f.d[0] == 0x409042e4u && f.d[1] == 0x42e443c8u && f.d[2] == 0x43c84090u, "bfloat16, interleaved: %08x %08x %08x", f.d[0], f.d[1], f.d[2]);
    nz.dtype = PJD_DT_F16;
    f = pjd_pad_fill(nz, true, fill, nullptr);
    CHECK(f.d[0] == 0x57205720u && f.d[1] == 0x44804480u && f.d[2] == 0x5e445e44u, "binary16, planar: %08x %08x %08x", f.d[0], f.d[1], f.d[2]);
    const float value[3] = {0.0f, -2.0f, 3e-6f};                 // 3e-6: a binary16 subnormal, 50 units of 2^-24 (50.33 rounds down)
    f = pjd_pad_fill(nz, true, fill, value);
    CHECK(f.d[0] == 0u && f.d[1] == 0xc000c000u && f.d[2] == 0x00320032u, "the pad value, binary16: %08x %08x %08x", f.d[0], f.d[1], f.d[2]);
    CHECK(pjd_f32_to_dtype_bits(PJD_DT_F16, 65520.0f) == 0x7c00u && pjd_f32_to_dtype_bits(PJD_DT_BF16, 1.00390625f) == 0x3f80u && pjd_f32_to_dtype_bits(PJD_DT_BF16, 1.01171875f) == 0x3f82u,
          "rounding to nearest even");
}

// A colour map (pjd_batch_set_colour): the limits on both sides of their boundary in every slot, the records against the statement of
// include/pjd.h written out here, and the form -- the padded one with the identity window, orientation 1 and an all-zero pad where
// none was asked for -- whose other records are those of the same request with a neutral pad, orientation and window
static void coloured()
{
    const int checks0 = g_checks, bad0 = g_bad;
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    auto with_colour = [&](PjdResizeSpec s, size_t i, int slot, double v) {
        s.colour_set = true;
        PjdColour c; memcpy(c.m, ident, sizeof ident);
        s.colour.assign(s.pic.size(), c);
        if (slot >= 0) s.colour[i].m[slot] = v;
        return s;
    };
    const PjdResizeSpec base = plain_spec(3, 61, 45, 30, 20, true);
    expect(with_colour(base, 0, -1, 0), -2, "identity maps");
    for (int slot = 0; slot < 12; slot++) {
        const bool off = slot % 4 == 3;
        const double lim = off ? 4096.0 : 16.0;
        for (double sign : {1.0, -1.0}) {
            expect(with_colour(base, 1, slot, sign * lim), -2, "a value at the limit");
            expect(with_colour(base, 1, slot, sign * std::nextafter(lim, 2 * lim)), -2, "the next double quantises to the limit");
            expect(with_colour(base, 1, slot, sign * (lim + 1.0 / 65536.0)), 1, "the next quantised value");
        }
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY, 1e300, -1e300}) expect(with_colour(base, 2, slot, bad), 2, "not finite, or far beyond");
        PjdDevColour rec;
        PjdColour c; memcpy(c.m, ident, sizeof ident); c.m[slot] = lim + 1.0 / 65536.0;
        const char *text = pjd_colour_quantise(c.m, rec);
        CHECK(text && std::string(text) == (off ? "an offset is beyond 4096 levels in magnitude" : "a weight is beyond 16 in magnitude"), "the text of slot %d: %s", slot, text ? text : "(accepted)");
    }
    {   // grey: refused for the batch as a whole
        PjdResizeSpec g = with_colour(base, 0, -1, 0);
        g.channels = 1;
        expect(g, -1, "a grey batch");
    }
    // the records: llrint(m * 65536), ties to even; the flag where that is the identity, also for a matrix that only rounds to it
    {
        PjdResizeSpec s = with_colour(base, 0, -1, 0);
        const double m1[12] = {0.299, 0.587, 0.114, 0, -0.5, 1.25, 1.0 / 131072, -12.75, 3.0 / 131072, -1.0 / 131072, 16, 4096};
        memcpy(s.colour[1].m, m1, sizeof m1);
        s.colour[2].m[0] = 1.0 + 1.0 / 262144; s.colour[2].m[7] = -1.0 / 262144;       // a quarter of a unit: rounds to the identity
        PjdResizeWork w;
        const PjdResizeFault f = pjd_resize_resolve(s, w);
        CHECK(f.text.empty() && w.form.coloured && w.colour.size() == 3, "the request resolves: %s", f.text.c_str());
        if (w.colour.size() == 3) {
            const int32_t want[12] = {19595, 38470, 7471, 0, -32768, 81920, 0, -835584, 2, 0, 1048576, 268435456};
            for (int c = 0; c < 3; c++) {
                for (int k = 0; k < 3; k++) CHECK(w.colour[1].q[c][k] == want[4 * c + k], "q[%d][%d] = %d", c, k, w.colour[1].q[c][k]);
                CHECK(w.colour[1].o[c] == want[4 * c + 3], "o[%d] = %d", c, w.colour[1].o[c]);
            }
            CHECK(w.colour[0].flags == PJD_COL_IDENTITY && w.colour[1].flags == 0 && w.colour[2].flags == PJD_COL_IDENTITY && w.colour[2].q[0][0] == 65536 && w.colour[2].o[1] == 0, "the identity flag");
        }
    }
    // the form, over every filter and layout and with a real pad, orientation and window under it
    int n = 0;
    for (int filter : {PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC})
        for (int planar = 0; planar < 2; planar++)
            for (int shaped = 0; shaped < 2; shaped++, n++) {
                PjdResizeSpec s = with_filter(plain_spec(3, 61, 45, 30, 20, planar != 0), filter);
                if (shaped) {
                    s = with_pad(s, 1, pjd_resize_pad{2, 1, 3, 0});
                    s.ori_set = true; s.orientation.assign(3, 1); s.orientation[2] = 6;
                    s = with_window(s, 0, pjd_resize_window{3, 4, 40, 30, 0, 0, 0, 0, PJD_RW_HFLIP, 0});
                }
                PjdResizeSpec neutral = s;                   // the same request with every array given: what the coloured one must equal but for its own records
                if (!shaped) { neutral.pad_set = true; neutral.pad.assign(3, pjd_resize_pad{}); neutral.ori_set = true; neutral.orientation.assign(3, 1); neutral.win_set = true; neutral.win.assign(3, pjd_resize_window{}); }
                PjdResizeWork plain, col;
                CHECK(pjd_resize_resolve(neutral, plain).text.empty(), "the uncoloured request resolves");
                const PjdResizeFault f = pjd_resize_resolve(with_colour(s, 1, 5, 0.5), col);
                CHECK(f.text.empty() && col.form.coloured && col.form.padded && col.form.oriented && col.form.windowed && !col.form.warp, "member %d: the form of a coloured request", n);
                CHECK(col.win.size() == 3 && col.pad.size() == 3 && col.line_prefix.size() == 4 && col.colour.size() == 3, "member %d: the records of a coloured request", n);
                CHECK(col.form.tiles == plain.form.tiles && col.form.lds == plain.form.lds && col.form.lines == (shaped ? plain.form.lines : 0u), "member %d: tiles, LDS and border lines", n);
                CHECK(same(col.recs, plain.recs) && same(col.tile_prefix, plain.tile_prefix) && same(col.aa, plain.aa) && same(col.tab, plain.tab), "member %d: work list and tables", n);
                if (shaped) CHECK(same(col.win, plain.win) && same(col.pad, plain.pad) && same(col.line_prefix, plain.line_prefix), "member %d: windows and canvases", n);
                else for (size_t i = 0; i < 3; i++) {
                    const PjdDevResizePad &c = col.pad[i];
                    CHECK(c.W == 30 && c.H == 20 && c.left == 0 && c.top == 0 && c.cw == 30 && c.ch == 20 && col.line_prefix[i] == 0 && col.win[i].flags == 0 && col.win[i].w == 61 && col.win[i].vh == 20, "member %d: the neutral records of picture %zu", n, i);
                }
                CHECK(!plain.form.coloured && plain.colour.empty(), "a request without a map has no colour record");
            }
    // views: the fault names view and picture
    {
        PjdResizeSpec s = with_colour(base, 2, 3, -4097.0);
        s.view_pic = {2, 0, 0};
        PjdResizeWork w;
        const PjdResizeFault f = pjd_resize_resolve(s, w);
        CHECK(!f.state && f.picture == 2 && f.text == "view 2 (picture 0): an offset is beyond 4096 levels in magnitude", "text: %s", f.text.c_str());
    }
    printf("coloured: %d checks, %d failed\n", g_checks - checks0, g_bad - bad0);
}

int main()
{
    limits();
    coloured();
    int members = 0;
    for (int pads = 0; pads < 3; pads++) for (int oris = 0; oris < 3; oris++) for (int wins = 0; wins < 3; wins++)
        for (int filter : {PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC})
            for (int planar = 0; planar < 2; planar++) family(pads, oris, wins, filter, planar != 0, 1000u + (uint32_t)members++);
    layout_and_fill();
    printf("%d members of the family, %d checks failed\n", members, g_bad);
    if (g_bad) return 1;
    printf("no sanitizer report\n");
    return 0;
}
