// resize_views_host.cpp -- the resolver of the resample work list (pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp) under requests as
// pjd_batch_set_views makes them, on the CPU, under the sanitizers:
//   1. a request whose `pic` entries repeat and permute their sources resolves, output by output, to the records the same pictures
//      resolve to ONE AT A TIME -- no record depends on its neighbours but for its place in the prefix sums and in the weight table;
//   2. the records of a V-view request equal those of the same request grown setter by setter, in the setters' call order;
//   3. the prefix sums over tiles and border lines are made in 64 bits and refused from 2^31 on, on both sides of that boundary and at
//      2^32 and beyond, where a 32-bit sum would have wrapped into range; and the fault texts name the view.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__host__= -D__device__= -o resize_views_host
//         tools/resize_views_host.cpp pim-jpeg-decoder_amd/csrc/pjd_resize_plan.cpp && ./resize_views_host
//
// tests/test_views_cpu.py builds and runs it.  Prints `no sanitizer report` at the end; exit status 1 where a check failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../pim-jpeg-decoder_amd/csrc/pjd_resize_plan.h"

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_bad++ < 20) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t g_seed = 7;
static uint32_t rnd(uint32_t n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }   // 0 .. n-1

template <class T> static bool same_bytes(const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// the pictures of a batch, as the back end leaves them in the intermediate buffer: ragged sizes, back to back
struct Source { uint64_t off; uint32_t sw, sh; };
static std::vector<Source> sources(size_t n, bool planar)
{
    std::vector<Source> s;
    uint64_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t sw = 17 + rnd(300), sh = 9 + rnd(200);
        s.push_back({off, sw, sh});
        off += (3ull * sw * sh + 255) & ~255ull;
    }
    (void)planar;
    return s;
}

// one view's whole request: everything a caller can say about one output
struct View {
    uint32_t pic;
    uint32_t out_w, out_h;
    pjd_resize_pad pad;
    uint8_t ori;
    pjd_resize_window win;
};

static View random_view(const std::vector<Source> &src, bool table)
{
    View v{};
    v.pic = rnd((uint32_t)src.size());
    const Source &s = src[v.pic];
    v.ori = (uint8_t)(1 + rnd(8));
    // the content (Q's target before the transpose) between 7 x 5 and 300 x 96: several column tiles, ragged lane groups
    uint32_t tw = 7 + rnd(294), th = 5 + rnd(92);
    if (table) { tw = std::max(tw, (s.sw + 15) / 16); th = std::max(th, (s.sh + 15) / 16); }    // inside the 16x limit
    v.pad = rnd(3) ? pjd_resize_pad{rnd(6), rnd(5), rnd(7), rnd(4)} : pjd_resize_pad{};
    const bool t = v.ori >= 5;
    v.out_w = (t ? th : tw) + v.pad.left + v.pad.right;
    v.out_h = (t ? tw : th) + v.pad.top + v.pad.bottom;
    if (rnd(3)) {
        const uint32_t w = std::max<uint32_t>(1u, s.sw - rnd(s.sw / 2)), h = std::max<uint32_t>(1u, s.sh - rnd(s.sh / 2));
        v.win = pjd_resize_window{rnd(s.sw - w + 1), rnd(s.sh - h + 1), w, h, 0, 0, 0, 0, rnd(2), 0};
        if (rnd(2)) { v.win.vw = tw + rnd(9); v.win.ox = rnd(v.win.vw - tw + 1); }
    }
    return v;
}

// the request the setters of pjd_api.hip have built once `level` of them were called: 0 set_resize, 1 + set_resize_pad, 2 + set_orientation,
// 3 + set_resize_window, 4 + set_resize_filter
static PjdResizeSpec spec_of(const std::vector<Source> &src, const std::vector<View> &views, bool planar, uint32_t channels, int filter, int level, bool named)
{
    PjdResizeSpec s;
    s.planar = planar; s.channels = channels;
    uint64_t dst = 0;
    for (const View &v : views) {
        const Source &p = src[v.pic];
        s.pic.push_back(PjdResizePicture{p.off, dst, p.sw, p.sh, planar ? p.sw : 3 * p.sw});
        s.out_w.push_back(v.out_w); s.out_h.push_back(v.out_h);
        dst += ((uint64_t)channels * v.out_w * v.out_h + 255) & ~255ull;
        if (named) s.view_pic.push_back(v.pic);
    }
    if (level >= 1) { s.pad_set = true; for (const View &v : views) s.pad.push_back(v.pad); }
    if (level >= 2) { s.ori_set = true; for (const View &v : views) s.orientation.push_back(v.ori); }
    if (level >= 3) { s.win_set = true; for (const View &v : views) s.win.push_back(v.win); }
    if (level >= 4) { s.filter_set = true; s.filter = filter; }
    return s;
}

// 1: repeated and permuted sources
static void repeats_and_permutes(int filter, bool planar, uint32_t channels)
{
    const bool table = filter != PJD_RESIZE_BILINEAR;
    const std::vector<Source> src = sources(5, planar);
    std::vector<View> views;
    for (int k = 0; k < 23; k++) views.push_back(random_view(src, table));
    views[3] = views[11];                                      // two views that are the same request, apart
    views[7].pic = views[8].pic = views[9].pic = 2;            // three neighbours of one source ...
    for (int k = 7; k <= 9; k++) { views[k].win = pjd_resize_window{}; views[k].pad = pjd_resize_pad{}; views[k].ori = 1; views[k].out_w = 40 + k; views[k].out_h = 30; }
    const PjdResizeSpec all = spec_of(src, views, planar, channels, filter, 4, true);
    PjdResizeWork W;
    const PjdResizeFault f = pjd_resize_resolve(all, W);
    CHECK(f.text.empty(), "the request of 23 views is refused: %s", f.text.c_str());
    if (!f.text.empty()) return;
    CHECK(W.recs.size() == views.size() && W.tile_prefix.size() == views.size() + 1, "sizes");
    CHECK(W.form.windowed && W.form.oriented && W.form.padded, "the request has every record kind");
    uint32_t tiles = 0, lines = 0;
    for (size_t v = 0; v < views.size(); v++) {
        // the same picture, alone, with the same setters -- in the most general form, which is the one the 23 run
        std::vector<View> one{views[v]};
        PjdResizeSpec s1 = spec_of(src, one, planar, channels, filter, 4, false);
        s1.pic[0].dst_off = all.pic[v].dst_off;
        PjdResizeWork w1;
        const PjdResizeFault f1 = pjd_resize_resolve(s1, w1);
        CHECK(f1.text.empty(), "view %zu alone is refused: %s", v, f1.text.c_str());
        if (!f1.text.empty()) continue;
        CHECK(same_bytes(W.recs[v], w1.recs[0]), "view %zu: the resize record differs from the picture's alone", v);
        CHECK(W.recs[v].src_off == src[views[v].pic].off && W.recs[v].sw == src[views[v].pic].sw, "view %zu reads its own picture", v);
        // a picture alone may take a lesser form (no window, no pad): its records are then the defaults the general form writes out
        if (w1.form.windowed) CHECK(same_bytes(W.win[v], w1.win[0]), "view %zu: the window record differs", v);
        else CHECK(same_bytes(W.win[v], pjd_resize_win_identity(w1.recs[0])), "view %zu: the window record is not the identity", v);
        if (w1.form.padded) CHECK(same_bytes(W.pad[v], w1.pad[0]), "view %zu: the canvas record differs", v);
        else CHECK(W.pad[v].W == views[v].out_w && W.pad[v].H == views[v].out_h && W.pad[v].left == 0 && W.pad[v].top == 0 && W.pad[v].cw == views[v].out_w && W.pad[v].ch == views[v].out_h, "view %zu: the canvas record is not the whole canvas", v);
        CHECK(W.tile_prefix[v] == tiles && W.tile_prefix[v + 1] - W.tile_prefix[v] == w1.form.tiles, "view %zu: tiles", v);
        tiles += w1.form.tiles;
        CHECK(W.line_prefix[v] == lines && W.line_prefix[v + 1] - W.line_prefix[v] == w1.form.lines, "view %zu: border lines %u, alone %u", v, W.line_prefix[v + 1] - W.line_prefix[v], w1.form.lines);
        lines += w1.form.lines;
        if (table) {
            // the weights are the picture's own, wherever the shared table keeps them
            const PjdDevResizeAA &a = W.aa[v], &b = w1.aa[0];
            CHECK(a.x_taps == b.x_taps && a.y_taps == b.y_taps, "view %zu: tap counts", v);
            const uint32_t vw = W.win[v].vw, vh = W.win[v].vh;
            bool eq = a.x_taps == b.x_taps && a.y_taps == b.y_taps;
            for (uint32_t k = 0; eq && k < vw * (1u + a.x_taps); k++) eq = W.tab[a.x_tab + k] == w1.tab[b.x_tab + k];
            for (uint32_t k = 0; eq && k < vh * (1u + a.y_taps); k++) eq = W.tab[a.y_tab + k] == w1.tab[b.y_tab + k];
            CHECK(eq, "view %zu: the axis tables differ from the picture's alone", v);
            CHECK(W.form.lds >= w1.form.lds, "view %zu: the launch's LDS covers it", v);
        }
    }
    CHECK(W.form.tiles == tiles && W.form.lines == lines, "totals");
    // the same views in another order: every view keeps its records, the prefix sums follow the order
    std::vector<size_t> order(views.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = (k * 7 + 3) % order.size();      // 7 and 23 are coprime: a permutation
    std::vector<View> perm;
    for (size_t k : order) perm.push_back(views[k]);
    PjdResizeSpec ps = spec_of(src, perm, planar, channels, filter, 4, true);
    for (size_t k = 0; k < order.size(); k++) ps.pic[k].dst_off = all.pic[order[k]].dst_off;
    PjdResizeWork PW;
    CHECK(pjd_resize_resolve(ps, PW).text.empty(), "the permuted request is refused");
    for (size_t k = 0; k < order.size() && PW.recs.size() == order.size(); k++) {
        CHECK(same_bytes(PW.recs[k], W.recs[order[k]]) && same_bytes(PW.win[k], W.win[order[k]]) && same_bytes(PW.pad[k], W.pad[order[k]]), "permuted view %zu", k);
        CHECK(PW.tile_prefix[k + 1] - PW.tile_prefix[k] == W.tile_prefix[order[k] + 1] - W.tile_prefix[order[k]], "permuted view %zu: tiles", k);
    }
    CHECK(PW.form.tiles == W.form.tiles && PW.form.lines == W.form.lines && PW.form.lds == W.form.lds, "the permuted totals");
    // names in the request change no record
    PjdResizeWork U;
    CHECK(pjd_resize_resolve(spec_of(src, views, planar, channels, filter, 4, false), U).text.empty(), "the unnamed request is refused");
    CHECK(U.recs.size() == W.recs.size() && std::memcmp(U.recs.data(), W.recs.data(), W.recs.size() * sizeof(PjdDevResize)) == 0 && U.tab == W.tab && U.tile_prefix == W.tile_prefix, "view names changed a record");
}

// 2: setter by setter.  Views that every level accepts: no pad and no orientation change what a window is held against
static void grown(int filter, bool planar)
{
    const std::vector<Source> src = sources(4, planar);
    std::vector<View> views;
    for (int k = 0; k < 12; k++) {
        View v = random_view(src, filter != PJD_RESIZE_BILINEAR);
        v.win.vw = v.win.ox = 0;                               // the default virtual target: valid against any target
        views.push_back(v);
    }
    // as the setters of pjd_api.hip do: a copy of the batch's request takes the setter's array, is resolved, and becomes the request
    PjdResizeSpec spec = spec_of(src, views, planar, 3, filter, 0, true);
    PjdResizeWork prev;
    for (int level = 0; level <= 4; level++) {
        PjdResizeSpec next = spec;
        if (level == 1) { next.pad_set = true; for (const View &v : views) next.pad.push_back(v.pad); }
        if (level == 2) { next.ori_set = true; for (const View &v : views) next.orientation.push_back(v.ori); }
        if (level == 3) { next.win_set = true; for (const View &v : views) next.win.push_back(v.win); }
        if (level == 4) { next.filter_set = true; next.filter = filter; }
        PjdResizeWork w;
        const PjdResizeFault f = pjd_resize_resolve(next, w);
        CHECK(f.text.empty(), "level %d is refused: %s", level, f.text.c_str());
        CHECK(w.recs.size() == views.size(), "level %d: records", level);
        for (size_t v = 0; v < w.recs.size(); v++) CHECK(w.recs[v].src_off == src[views[v].pic].off && w.recs[v].dst_off == next.pic[v].dst_off, "level %d view %zu: offsets", level, v);
        spec = next;
        prev = w;
    }
    // ... against the whole request written down at once
    PjdResizeWork once;
    CHECK(pjd_resize_resolve(spec_of(src, views, planar, 3, filter, 4, true), once).text.empty(), "in one go");
    CHECK(once.recs.size() == prev.recs.size() && std::memcmp(once.recs.data(), prev.recs.data(), prev.recs.size() * sizeof(PjdDevResize)) == 0, "records");
    CHECK(once.win.size() == prev.win.size() && (once.win.empty() || std::memcmp(once.win.data(), prev.win.data(), prev.win.size() * sizeof(PjdDevResizeWin)) == 0), "windows");
    CHECK(once.pad.size() == prev.pad.size() && (once.pad.empty() || std::memcmp(once.pad.data(), prev.pad.data(), prev.pad.size() * sizeof(PjdDevResizePad)) == 0), "canvases");
    CHECK(once.tile_prefix == prev.tile_prefix && once.line_prefix == prev.line_prefix && once.tab == prev.tab, "prefix sums and tables");
}

// n views of one 8 x 8 picture, each tw x th
static PjdResizeSpec many(size_t n, uint32_t tw, uint32_t th, bool planar = false)
{
    PjdResizeSpec s;
    s.planar = planar;
    s.pic.assign(n, PjdResizePicture{0, 0, 8, 8, planar ? 8u : 24u});
    s.out_w.assign(n, tw); s.out_h.assign(n, th);
    s.view_pic.assign(n, 0u);
    return s;
}

static bool resolves(const PjdResizeSpec &s, std::string *text = nullptr, PjdResizeWork *out = nullptr)
{
    PjdResizeWork w;
    const PjdResizeFault f = pjd_resize_resolve(s, w);
    if (text) *text = f.text;
    if (out) *out = w;
    return f.text.empty();
}

static void prefix_sum_limits()
{
    const uint64_t per = 256ull * 8192ull;                      // tiles of a 65535 x 65535 target: ceil(65535 / 256) * ceil(65535 / 8) = 2^21
    CHECK(((65535 + PJD_RS_COLS - 1) / PJD_RS_COLS) * (uint64_t)((65535 + PJD_RS_ROWS - 1) / PJD_RS_ROWS) == per, "tiles of the largest target");
    std::string text;
    // ---- tiles: 2^31 - 1 is taken, 2^31 refused.  1023 views of 2^21 tiles, one of 255 x 8192, one of 8191: 2^31 - 1
    PjdResizeSpec s = many(1025, 65535, 65535);
    s.out_w[1023] = 255 * 256;                                  // 255 column tiles x 8192 row tiles
    s.out_w[1024] = 1; s.out_h[1024] = 8191 * 8;                // 1 x 8191
    PjdResizeWork w;
    CHECK(resolves(s, &text, &w), "2^31 - 1 tiles are refused: %s", text.c_str());
    CHECK(w.form.tiles == 0x7fffffffu && w.tile_prefix.back() == 0x7fffffffu && w.tile_prefix[1024] == 0x7fffffffu - 8191u, "the sum of 2^31 - 1 tiles: %u", w.form.tiles);
    for (size_t k = 1; k < w.tile_prefix.size(); k++) if (w.tile_prefix[k] < w.tile_prefix[k - 1]) { CHECK(false, "the tile prefix sum is not monotonic at %zu", k); break; }
    s.out_h[1024] = 65535;                                      // one tile more (8192 row tiles): 2^31
    CHECK(!resolves(s, &text) && text.find("too large for one launch") != std::string::npos, "2^31 tiles: %s", text.empty() ? "accepted" : text.c_str());
    // ---- at 2^32 and beyond a 32-bit sum would be back in range: 2048 views make exactly 2^32 (0 in 32 bits), 2049 make 2^21 more
    for (size_t n : {(size_t)2048, (size_t)2049, (size_t)65536}) {
        CHECK(((uint64_t)n * per) >> 32 != 0 && (uint32_t)((uint64_t)n * per) < (1u << 31), "the case wraps into range");
        CHECK(!resolves(many(n, 65535, 65535), &text) && text.find("too large for one launch") != std::string::npos, "%zu views of 2^21 tiles: %s", n, text.empty() ? "accepted" : text.c_str());
    }
    // ---- border lines: an interleaved view of out_h rows with a pad has out_h of them.  32768 views of 65535 rows and one of 32767: 2^31 - 1
    PjdResizeSpec p = many(32769, 4, 65535);
    p.pad_set = true; p.pad.assign(p.pic.size(), pjd_resize_pad{1, 0, 0, 0});
    p.out_h[32768] = 32767;
    CHECK(32768ull * 65535 + 32767 == (1ull << 31) - 1, "the arithmetic of the case");
    CHECK(resolves(p, &text, &w), "2^31 - 1 border lines are refused: %s", text.c_str());
    CHECK(w.form.lines == 0x7fffffffu && w.line_prefix.back() == 0x7fffffffu && w.line_prefix[32768] == 0x7fffffffu - 32767u, "the sum of the border lines: %u", w.form.lines);
    p.pad[7] = pjd_resize_pad{};                                // a view without a border has no line: room for one more row
    p.out_h[32768] = 32768;
    CHECK(resolves(p, &text, &w) && w.form.lines == 0x7fffffffu - 65534u, "a view without a border: %s", text.c_str());
    p.pad[7] = pjd_resize_pad{0, 1, 0, 0};
    CHECK(!resolves(p, &text) && text.find("canvases of this batch are too large") != std::string::npos, "2^31 border lines: %s", text.empty() ? "accepted" : text.c_str());
    // ... and past 2^32: 21846 planar views of 65535 rows have 3 * 21846 * 65535 = 2^32 + 65534 lines, 65534 in 32 bits
    PjdResizeSpec q = many(21846, 4, 65535, true);
    q.pad_set = true; q.pad.assign(q.pic.size(), pjd_resize_pad{1, 0, 0, 0});
    CHECK(3ull * 21846 * 65535 == (1ull << 32) + 65534, "the case wraps into range");
    CHECK(!resolves(q, &text) && text.find("canvases of this batch are too large") != std::string::npos, "2^32 + 65534 border lines: %s", text.empty() ? "accepted" : text.c_str());
}

static void names()
{
    std::string text;
    PjdResizeSpec s = many(6, 20, 10);
    s.view_pic = {4, 4, 0, 2, 2, 1};
    s.out_w[3] = 0;
    CHECK(!resolves(s, &text) && text == "view 3 (picture 2): target width and height must be 1..65535", "%s", text.c_str());
    s.out_w[3] = 20;
    s.ori_set = true; s.orientation = {1, 1, 1, 1, 9, 1};
    CHECK(!resolves(s, &text) && text.rfind("view 4 (picture 2): ", 0) == 0, "%s", text.c_str());
    s.orientation[4] = 1;
    s.pad_set = true; s.pad.assign(6, pjd_resize_pad{}); s.pad[5] = pjd_resize_pad{10, 0, 10, 0};
    CHECK(!resolves(s, &text) && text.rfind("view 5 (picture 1): left + right", 0) == 0, "%s", text.c_str());
    s.pad[5] = pjd_resize_pad{};
    s.win_set = true; s.win.assign(6, pjd_resize_window{}); s.win[0] = pjd_resize_window{7, 0, 2, 8, 0, 0, 0, 0, 0, 0};
    CHECK(!resolves(s, &text) && text.rfind("view 0 (picture 4): the window is not inside", 0) == 0, "%s", text.c_str());
    s.win[0] = pjd_resize_window{};
    s.filter_set = true; s.filter = PJD_RESIZE_ANTIALIAS;
    s.pic[1].sw = 400; s.pic[1].src_stride = 1200;             // 400 columns to 20: past 16x
    CHECK(!resolves(s, &text) && text.find("view 1 (picture 4) is more than 16x its target") == 0, "%s", text.c_str());
    s.win[1] = pjd_resize_window{0, 0, 400, 8, 0, 0, 0, 0, 1, 0};
    CHECK(!resolves(s, &text) && text.find("the window of view 1 (picture 4) is more than 16x") == 0, "%s", text.c_str());
    // without names the same faults name the picture, as they always did
    s.view_pic.clear();
    CHECK(!resolves(s, &text) && text.find("the window of picture 1 is more than 16x") == 0, "%s", text.c_str());
    CHECK(pjd_resize_output_name(s, 3) == "picture 3", "name");
}

int main()
{
    for (int filter : {PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC})
        for (int planar = 0; planar < 2; planar++) {
            repeats_and_permutes(filter, planar != 0, 3);
            grown(filter, planar != 0);
        }
    repeats_and_permutes(PJD_RESIZE_ANTIALIAS, true, 1);        // a grey batch: one plane, always the padded form
    prefix_sum_limits();
    names();
    printf("%d checks, %d checks failed\n", g_checks, g_bad);
    printf("no sanitizer report\n");
    return g_bad ? 1 : 0;
}
