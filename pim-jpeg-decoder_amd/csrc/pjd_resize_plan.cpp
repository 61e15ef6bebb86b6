// pjd_resize_plan.cpp -- the resample work list as a function of the request (pjd_resize_plan.h).  Host only, no HIP call.
#include "pjd_resize_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

namespace {

PjdResizeFault fault_at(const PjdResizeSpec &spec, size_t i, const char *text)
{
    return PjdResizeFault{pjd_resize_output_name(spec, i) + ": " + text, (int)i};
}

PjdResizeFault fault_of(const PjdResizeSpec &spec, const char *fmt, size_t i)        // a text that names its picture itself (%s)
{
    char buf[240];
    std::snprintf(buf, sizeof buf, fmt, pjd_resize_output_name(spec, i).c_str());
    return PjdResizeFault{buf, (int)i};
}

// The weight table of a table-driven filter: one axis table per distinct (source length, target length) of the batch -- the pictures
// of a data set share a few -- each dn heads `first | count << 16`, then taps x dn weights, tap-major, 0 behind a sample's own count
// (pjd_internal.h).  The bicubic filter has weights of either sign, kept as the bit patterns of int32, and its kernel's 32-bit
// accumulators hold only while sum |q_j| <= PJD_BICUBIC_MAX_GAIN (include/pjd.h): `gain` is the largest such sum of the axis.
struct Axis { uint32_t off, taps, gain; };
struct AxisTables {
    const bool cubic;
    const uint32_t max_taps;
    std::vector<uint32_t> &tab;
    std::map<std::pair<uint32_t, uint32_t>, Axis> axes;
    AxisTables(int filter, std::vector<uint32_t> &t) : cubic(filter == PJD_RESIZE_BICUBIC), max_taps(cubic ? PJD_BICUBIC_MAX_TAPS : PJD_AA_MAX_TAPS), tab(t) {}
    Axis axis(uint32_t sn, uint32_t dn)
    {
        auto it = axes.find({sn, dn});
        if (it != axes.end()) return it->second;
        const size_t base = tab.size();
        const uint32_t bound = ((cubic ? 4u : 2u) * std::max(sn, dn) + dn - 1u) / dn;   // no sample has more taps than ceil(2 * S / dn), bicubic ceil(4 * S / dn) (include/pjd.h)
        const uint32_t cap = std::min<uint32_t>(std::max<uint32_t>(bound, 1u), max_taps);
        tab.resize(base + (size_t)dn * (1u + cap), 0u);
        uint32_t taps = 0, gain = 0, w[PJD_BICUBIC_MAX_TAPS];
        static_assert(PJD_BICUBIC_MAX_TAPS >= PJD_AA_MAX_TAPS, "one array for both filters");
        for (uint32_t i = 0; i < dn; i++) {
            uint32_t first, sum = 0;
            const uint32_t cnt = std::min(cubic ? pjd_resize_bicubic_taps_calc(sn, dn, i, first, (int32_t *)w) : pjd_resize_aa_taps_calc(sn, dn, i, first, w), cap);
            tab[base + i] = first | (cnt << 16);
            for (uint32_t t = 0; t < cnt; t++) {
                tab[base + (size_t)(t + 1u) * dn + i] = w[t];
                sum += (int32_t)w[t] < 0 ? 0u - w[t] : w[t];
            }
            taps = std::max(taps, cnt);
            gain = std::max(gain, sum);
        }
        tab.resize(base + (size_t)dn * (1u + taps));       // the rows no sample reaches are dropped
        return axes[{sn, dn}] = Axis{(uint32_t)base, taps, gain};
    }
};

uint64_t warp_tiles_of(uint32_t tw, uint32_t th) { return (uint64_t)((tw + PJD_WARP_COLS - 1) / PJD_WARP_COLS) * ((th + PJD_WARP_ROWS - 1) / PJD_WARP_ROWS); }
uint64_t tiles_of(uint32_t tw, uint32_t th) { return (uint64_t)((tw + PJD_RS_COLS - 1) / PJD_RS_COLS) * ((th + PJD_RS_ROWS - 1) / PJD_RS_ROWS); }

// binary32 -> binary16 bits, round to nearest even, subnormals kept, overflow to infinity (the host side of PJD_DT_F16; the device
// converts in hardware, tests/test_gpu_normalize.py holds the two together)
uint16_t f32_to_f16_bits(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (a < 0x38800000u) {                                 // below 2^-14: a subnormal result, in units of 2^-24
        const uint32_t e = a >> 23;
        if (e < 102u) return (uint16_t)sign;               // below 2^-25: zero
        const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;      // 14..24
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return (uint16_t)(sign | q);
    }
    const uint32_t r = a - 0x38000000u;                    // exponent rebiased from 127 to 15
    uint32_t q = r >> 13;
    const uint32_t rem = r & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) q++;
    if (q > 0x7c00u) q = 0x7c00u;
    return (uint16_t)(sign | q);                           // a carry out of the mantissa runs into the exponent: 0x7c00 is infinity
}

uint64_t blur_tiles_of(uint32_t tw, uint32_t th) { return (uint64_t)((tw + PJD_BLUR_COLS - 1) / PJD_BLUR_COLS) * ((th + PJD_BLUR_ROWS - 1) / PJD_BLUR_ROWS); }

// The blur launch behind a resolved request (pjd_batch_set_blur): U of every output moves into the blur intermediate -- the packed layout
// of the uint8 outputs, which the resample's (or warp's) records then write -- and one blur record per output takes it from there to the
// final range.  The tap table: row 0 is the one tap {65536}, which every output without a blur and every table whose only non-zero tap is
// the centre reads; behind it one row per distinct (ksize, sigma), in the order the outputs name them.  The entries were checked before.
PjdResizeFault blur_stage(const PjdResizeSpec &spec, PjdResizeWork &out)
{
    if (!spec.blur_set) return PjdResizeFault{};
    const size_t n = spec.pic.size();
    const PjdPackedLayout lay = pjd_packed_layout(spec.out_w.data(), spec.out_h.data(), n, 1, spec.channels);
    out.blur.resize(n); out.blur_prefix.resize(n + 1);
    out.blur_taps.assign(1, 65536u);
    std::map<std::pair<uint32_t, uint64_t>, uint32_t> rows;           // (ksize, the bits of sigma) -> the row's offset; 0: the identity
    uint64_t tiles = 0;
    uint32_t r_max = 0;
    for (size_t i = 0; i < n; i++) {
        const pjd_blur &e = spec.blur[i];
        uint32_t off = 0;
        if (e.ksize > 1u) {
            uint64_t bits;
            std::memcpy(&bits, &e.sigma, 8);
            auto it = rows.find({e.ksize, bits});
            if (it != rows.end()) off = it->second;
            else {
                uint32_t q[PJD_BLUR_MAX_TAPS];
                pjd_blur_taps_calc(e.ksize, e.sigma, q);
                if (q[e.ksize / 2u] != 65536u) {           // the taps sum to 65536: the centre holds all of it, or the table blurs
                    off = (uint32_t)out.blur_taps.size();
                    out.blur_taps.insert(out.blur_taps.end(), q, q + e.ksize);
                }
                rows[{e.ksize, bits}] = off;
            }
        }
        out.blur[i] = PjdDevBlur{lay.off[i], spec.pic[i].dst_off, spec.out_w[i], spec.out_h[i], e.ksize, off, off ? 0u : PJD_BLUR_IDENTITY,
                                 (spec.out_w[i] + PJD_BLUR_COLS - 1) / PJD_BLUR_COLS};
        out.recs[i].dst_off = lay.off[i];
        if (off) r_max = std::max(r_max, e.ksize / 2u);
        out.blur_prefix[i] = (uint32_t)tiles;
        tiles += blur_tiles_of(spec.out_w[i], spec.out_h[i]);
        if (tiles >= (1ull << 31)) return PjdResizeFault{"the targets of this batch are too large for one launch", -1};
    }
    out.blur_prefix[n] = out.form.blur_tiles = (uint32_t)tiles;
    out.form.blurred = true;
    out.form.blur_lds = pjd_blur_lds(r_max, spec.channels);
    out.form.blur_buf_bytes = lay.buf_bytes;
    return PjdResizeFault{};
}

}  // namespace

const char *pjd_blur_fault(const pjd_blur *blur)
{
    if (!blur) return "null record";
    if (blur->reserved_ != 0) return "reserved_ must be 0";
    if (blur->ksize == 0) return blur->sigma == 0.0 ? nullptr : "sigma must be 0 where ksize == 0 (no blur)";
    if (blur->ksize > PJD_BLUR_MAX_TAPS) return "ksize is beyond PJD_BLUR_MAX_TAPS";
    if ((blur->ksize & 1u) == 0) return "ksize must be odd";
    if (!std::isfinite(blur->sigma) || !(blur->sigma > 0.0)) return "sigma must be finite and greater than 0";
    return nullptr;
}

// include/pjd.h, TAPS, term by term.  w[r] = exp(-0) = 1 and every other w is at most 1, so q[r] is the largest tap, at least
// 65536 / ksize, and the correction -- at most half a unit per tap -- cannot take it below zero.
void pjd_blur_taps_calc(uint32_t ksize, double sigma, uint32_t *q)
{
    const uint32_t r = ksize / 2u;
    double w[PJD_BLUR_MAX_TAPS], t = 0.0;
    for (uint32_t j = 0; j < ksize; j++) {
        const double d = ((double)j - (double)r) / sigma;
        w[j] = std::exp(-0.5 * (d * d));
        t += w[j];
    }
    int64_t sum = 0;
    for (uint32_t j = 0; j < ksize; j++) {
        q[j] = (uint32_t)std::llrint(w[j] / t * 65536.0);
        sum += q[j];
    }
    q[r] = (uint32_t)((int64_t)q[r] + 65536 - sum);
}

std::string pjd_resize_output_name(const PjdResizeSpec &spec, size_t i)
{
    char buf[64];
    if (i < spec.view_pic.size()) std::snprintf(buf, sizeof buf, "view %zu (picture %u)", i, spec.view_pic[i]);
    else std::snprintf(buf, sizeof buf, "picture %zu", i);
    return buf;
}

const char *pjd_resize_window_fault(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const pjd_resize_window *win, int filter)
{
    if (sw == 0 || sw > 65535u || sh == 0 || sh > 65535u || tw == 0 || tw > 65535u || th == 0 || th > 65535u) return "picture and target sizes must be 1..65535";
    if (!win) return "null record";
    if (filter != PJD_RESIZE_BILINEAR && filter != PJD_RESIZE_ANTIALIAS && filter != PJD_RESIZE_BICUBIC) return "unknown filter (PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS or PJD_RESIZE_BICUBIC)";
    if ((win->w == 0) != (win->h == 0)) return "an empty window (w and h are both 0 for the whole picture, or both at least 1)";
    if (win->w == 0 && (win->x != 0 || win->y != 0)) return "x and y must be 0 where w == h == 0 (the whole picture)";
    const uint64_t w = win->w ? win->w : sw, h = win->h ? win->h : sh;
    if ((uint64_t)win->x + w > sw || (uint64_t)win->y + h > sh) return "the window is not inside the picture at its decode size";
    if (win->vw > 65535u || win->vh > 65535u) return "the virtual target must be at most 65535 x 65535";
    const uint64_t vw = win->vw ? win->vw : tw, vh = win->vh ? win->vh : th;
    if ((uint64_t)win->ox + tw > vw || (uint64_t)win->oy + th > vh) return "the delivered columns and rows are not inside the virtual target";
    if (win->flags & ~PJD_RW_HFLIP) return "unknown flag bits";
    if (win->reserved_ != 0) return "reserved_ must be 0";
    if (filter != PJD_RESIZE_BILINEAR && (w > 16u * vw || h > 16u * vh)) return "the window is more than 16x its virtual target on an axis (PJD_RESIZE_ANTIALIAS, PJD_RESIZE_BICUBIC)";
    return nullptr;
}

// The sums are 64-bit: no record wraps into range.
const char *pjd_resize_pad_fault(uint32_t out_w, uint32_t out_h, const pjd_resize_pad *pad)
{
    if (out_w == 0 || out_w > 65535u || out_h == 0 || out_h > 65535u) return "the canvas must be 1..65535 x 1..65535";
    if (!pad) return "null record";
    if ((uint64_t)pad->left + pad->right >= out_w) return "left + right leaves no column of content (it must be less than out_w)";
    if ((uint64_t)pad->top + pad->bottom >= out_h) return "top + bottom leaves no row of content (it must be less than out_h)";
    return nullptr;
}

// The limits are those of include/pjd.h, checked on the quantised values: |a| <= 16 * 2^40 for the four linear coefficients (16 source
// pixels per target pixel, the 16x of the table-driven filters), |a| <= 2^18 * 2^40 for the two translations.  m * 2^40 is exact in
// binary64 (a power of two), llrint rounds it to nearest even once; the magnitude is bounded before the conversion, so it is defined.
const char *pjd_warp_quantise(const double m[6], PjdDevWarp &out)
{
    int64_t a[6];
    for (int k = 0; k < 6; k++) {
        if (!std::isfinite(m[k])) return "the matrix has a value that is not finite";
        const bool shift = k == 2 || k == 5;
        if (std::fabs(m[k]) > (shift ? 262145.0 : 17.0)) return shift ? "a translation is beyond 2^18 pixels in magnitude" : "a coefficient of the linear part is beyond 16 in magnitude";
        a[k] = (int64_t)std::llrint(std::ldexp(m[k], 40));
        const int64_t lim = shift ? (int64_t)1 << 58 : (int64_t)1 << 44;
        if (a[k] > lim || a[k] < -lim) return shift ? "a translation is beyond 2^18 pixels in magnitude" : "a coefficient of the linear part is beyond 16 in magnitude";
    }
    out = PjdDevWarp{a[0], a[1], 2 * a[2] - ((int64_t)1 << 40), a[3], a[4], 2 * a[5] - ((int64_t)1 << 40)};
    return nullptr;
}

const char *pjd_resize_affine_fault(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const double m[6])
{
    if (sw == 0 || sw > 65535u || sh == 0 || sh > 65535u || tw == 0 || tw > 65535u || th == 0 || th > 65535u) return "picture and target sizes must be 1..65535";
    if (!m) return "null matrix";
    PjdDevWarp rec;
    return pjd_warp_quantise(m, rec);
}

const char *pjd_resize_affine_excludes(const PjdResizeSpec &spec)
{
    return spec.pad_set ? "set_resize_pad" : spec.ori_set ? "set_orientation" : spec.win_set ? "set_resize_window" : spec.filter_set ? "set_resize_filter" : nullptr;
}

// The limits are those of include/pjd.h, checked on the quantised values as the warp's are: |q| <= 16 * 2^16 for the nine weights,
// |o| <= 4096 * 2^16 for the three offsets.  m * 65536 is exact in binary64, llrint rounds it to nearest even once; the magnitude is
// bounded before the conversion, so it is defined.
const char *pjd_colour_quantise(const double m[12], PjdDevColour &out)
{
    int32_t v[12];
    for (int k = 0; k < 12; k++) {
        if (!std::isfinite(m[k])) return "the matrix has a value that is not finite";
        const bool offset = (k & 3) == 3;
        const char *beyond = offset ? "an offset is beyond 4096 levels in magnitude" : "a weight is beyond 16 in magnitude";
        if (std::fabs(m[k]) > (offset ? 4097.0 : 17.0)) return beyond;
        const long long q = std::llrint(std::ldexp(m[k], 16)), lim = offset ? 1ll << 28 : 1ll << 20;
        if (q > lim || q < -lim) return beyond;
        v[k] = (int32_t)q;
    }
    out = PjdDevColour{};
    bool identity = true;
    for (int c = 0; c < 3; c++) {
        for (int k = 0; k < 3; k++) { out.q[c][k] = v[4 * c + k]; identity = identity && v[4 * c + k] == (c == k ? 65536 : 0); }
        out.o[c] = v[4 * c + 3]; identity = identity && v[4 * c + 3] == 0;
    }
    out.flags = identity ? PJD_COL_IDENTITY : 0u;
    return nullptr;
}

PjdResizeFault pjd_resize_resolve(const PjdResizeSpec &spec, PjdResizeWork &out)
{
    out = PjdResizeWork{};
    PjdResizeForm &form = out.form;
    const size_t n = spec.pic.size();
    const bool table = spec.filter == PJD_RESIZE_ANTIALIAS || spec.filter == PJD_RESIZE_BICUBIC;
    if (!table && spec.filter != PJD_RESIZE_BILINEAR) return PjdResizeFault{"unknown filter (PJD_RESIZE_BILINEAR, PJD_RESIZE_ANTIALIAS or PJD_RESIZE_BICUBIC)", -1};
    for (size_t i = 0; i < n; i++)
        if (spec.out_w[i] == 0 || spec.out_w[i] > 65535u || spec.out_h[i] == 0 || spec.out_h[i] > 65535u) return fault_at(spec, i, "target width and height must be 1..65535");

    // A blur (pjd_batch_set_blur) is a launch behind either request below (blur_stage), never behind a pad: the border there is not
    // content, and a pad value has no 8-bit form
    if (spec.blur_set) {
        if (spec.pad_set) return PjdResizeFault{"a blur and set_resize_pad exclude each other on one batch (the border is not content)", -1};
        for (size_t i = 0; i < n; i++)
            if (const char *f = pjd_blur_fault(&spec.blur[i])) return fault_at(spec, i, f);
    }

    // A colour map (pjd_batch_set_colour) is a layer on either request below: one record per output beside the work list, and the form
    // with the fewest kernels -- the padded one (identity window, orientation 1 and an all-zero pad where none was asked for), or the warp
    if (spec.colour_set) {
        if (spec.channels != 3u) return PjdResizeFault{"a grey batch has no colour map (one plane: gain and offset are pjd_batch_set_normalize's)", -1};
        out.colour.resize(n);
        for (size_t i = 0; i < n; i++)
            if (const char *f = pjd_colour_quantise(spec.colour[i].m, out.colour[i])) return fault_at(spec, i, f);
        form.coloured = true;
    }

    // An affine map (pjd_batch_set_resize_affine) is the whole request: no pad, orientation, window or filter beside it -- each is a matrix
    // the caller multiplies in -- and a form of its own, one record per output beside the work list, in tiles of the warp launch.
    if (spec.affine_set) {
        if (const char *other = pjd_resize_affine_excludes(spec))
            return PjdResizeFault{std::string("an affine map and ") + other + " exclude each other on one batch (multiply it into the matrix)", -1, true};
        out.ct_w = spec.out_w; out.ct_h = spec.out_h;
        out.recs.resize(n); out.tile_prefix.resize(n + 1); out.warp.resize(n);
        uint64_t tiles = 0;
        for (size_t i = 0; i < n; i++) {
            const PjdResizePicture &p = spec.pic[i];
            if (const char *f = pjd_resize_affine_fault(p.sw, p.sh, spec.out_w[i], spec.out_h[i], spec.affine[i].m)) return fault_at(spec, i, f);
            pjd_warp_quantise(spec.affine[i].m, out.warp[i]);
            out.recs[i] = PjdDevResize{p.src_off, p.dst_off, p.sw, p.sh, p.src_stride, spec.out_w[i], spec.out_h[i], (spec.out_w[i] + PJD_WARP_COLS - 1) / PJD_WARP_COLS};
            out.tile_prefix[i] = (uint32_t)tiles;
            tiles += warp_tiles_of(spec.out_w[i], spec.out_h[i]);
            if (tiles >= (1ull << 31)) return PjdResizeFault{"the targets of this batch are too large for one launch", -1};
        }
        out.tile_prefix[n] = form.tiles = (uint32_t)tiles;
        form.warp = true;
        return blur_stage(spec, out);
    }

    // the content of every delivered picture: its canvas less its pad; a padded picture has a border line per canvas line
    out.ct_w = spec.out_w; out.ct_h = spec.out_h;
    std::vector<uint8_t> bordered(n, 0);
    uint64_t lines = 0;
    if (spec.pad_set)
        for (size_t i = 0; i < n; i++) {
            const pjd_resize_pad &p = spec.pad[i];
            if (const char *f = pjd_resize_pad_fault(spec.out_w[i], spec.out_h[i], &p)) return fault_at(spec, i, f);
            out.ct_w[i] -= p.left + p.right; out.ct_h[i] -= p.top + p.bottom;
            bordered[i] = p.left || p.top || p.right || p.bottom;
            if (bordered[i]) lines += (uint64_t)(spec.planar ? spec.channels : 1u) * spec.out_h[i];
            form.padded = form.padded || bordered[i];
        }
    // both prefix sums are made in 64 bits and refused from 2^31 on: with views (up to PJD_MAX_VIEWS outputs of up to 2^21 tiles each) a
    // request can pass 2^32, and nothing of it is narrowed to the kernels' 32-bit words before it has been refused here
    if (lines >= (1ull << 31)) return PjdResizeFault{"the canvases of this batch are too large for one launch", -1};

    // Q, the picture the resample computes: its target is the content with the axes swapped where the orientation transposes
    std::vector<uint32_t> ori(n, 0u), tw(out.ct_w), th(out.ct_h);
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t o = spec.ori_set ? spec.orientation[i] : 1u;
        if (o < 1u || o > 8u) return fault_at(spec, i, "the orientation must be 1..8");
        ori[i] = pjd_orient_flags(o);
        if (ori[i] & PJD_RWI_TRANSPOSE) std::swap(tw[i], th[i]);
        form.oriented = form.oriented || o != 1u;
        tiles += tiles_of(tw[i], th[i]);
    }
    if (tiles >= (1ull << 31)) return PjdResizeFault{"the targets of this batch are too large for one launch", -1};

    bool any_win = false;
    if (spec.win_set)
        for (size_t i = 0; i < n; i++) {
            const pjd_resize_window &w = spec.win[i];
            if (const char *f = pjd_resize_window_fault(spec.pic[i].sw, spec.pic[i].sh, tw[i], th[i], &w, PJD_RESIZE_BILINEAR)) return fault_at(spec, i, f);
            any_win = any_win || w.x || w.y || w.w || w.h || w.vw || w.vh || w.ox || w.oy || w.flags;
        }
    // the most general form a batch needs is the one it runs: a pad brings the oriented launch, an orientation the windowed one
    // a grey batch has the padded kernels alone (pjd_k_resize.hip): a picture without a pad is its whole canvas, and has no border line
    // a coloured batch likewise, for the same reason: the instantiation count
    if (spec.channels == 1u || form.coloured) form.padded = true;
    form.oriented = form.oriented || form.padded;
    form.windowed = form.oriented || any_win;

    // the records, as the kernels read them (pjd_internal.h)
    out.recs.resize(n); out.tile_prefix.resize(n + 1);
    if (form.windowed) out.win.resize(n);
    if (form.padded) { out.pad.resize(n); out.line_prefix.resize(n + 1); }
    for (size_t i = 0; i < n; i++) {
        const PjdResizePicture &p = spec.pic[i];
        PjdDevResize &r = out.recs[i];
        r = PjdDevResize{p.src_off, p.dst_off, p.sw, p.sh, p.src_stride, tw[i], th[i], (tw[i] + PJD_RS_COLS - 1) / PJD_RS_COLS};
        out.tile_prefix[i] = form.tiles;
        form.tiles += (uint32_t)tiles_of(tw[i], th[i]);
        if (form.windowed) {
            // every default resolved; the window's mirror composes with the orientation's tap mirror by exclusive-or
            const pjd_resize_window w = spec.win_set ? spec.win[i] : pjd_resize_window{};
            out.win[i] = PjdDevResizeWin{w.x, w.y, w.w ? w.w : r.sw, w.h ? w.h : r.sh, w.vw ? w.vw : r.tw, w.vh ? w.vh : r.th, w.ox, w.oy, w.flags ^ ori[i], 0u};
        }
        if (form.padded) {
            out.pad[i] = PjdDevResizePad{spec.out_w[i], spec.out_h[i], spec.pad_set ? spec.pad[i].left : 0u, spec.pad_set ? spec.pad[i].top : 0u, out.ct_w[i], out.ct_h[i], {0u, 0u}};
            out.line_prefix[i] = form.lines;
            if (bordered[i]) form.lines += (spec.planar ? spec.channels : 1u) * spec.out_h[i];
        }
    }
    out.tile_prefix[n] = form.tiles;
    if (form.padded) out.line_prefix[n] = form.lines;
    if (!table) return blur_stage(spec, out);

    // a table-driven filter.  A windowed picture takes the tables of its windowed axes, over the whole virtual target (tap index
    // ox + i', row length vw); one without is the windowed one with the identity window.  The limit is the window's (include/pjd.h)
    auto window = [&](size_t i) { return form.windowed ? out.win[i] : pjd_resize_win_identity(out.recs[i]); };
    for (size_t i = 0; i < n; i++) {
        const PjdDevResizeWin w = window(i);
        if (w.w > 16u * w.vw || w.h > 16u * w.vh)
            return fault_of(spec, form.windowed ? "the window of %s is more than 16x its virtual target on an axis (pre-scale with PJD_F_SCALE_*)"
                                                : "%s is more than 16x its target on an axis at its decode size (pre-scale with PJD_F_SCALE_*)", i);
    }
    AxisTables tables(spec.filter, out.tab);
    out.aa.resize(n);
    for (size_t i = 0; i < n; i++) {
        const PjdDevResize &r = out.recs[i];
        const PjdDevResizeWin w = window(i);
        if (out.tab.size() + ((size_t)w.vw + w.vh) * (1u + tables.max_taps) >= (1ull << 31)) return PjdResizeFault{"the weight table of this batch is too large", -1};
        const Axis x = tables.axis(w.w, w.vw), y = tables.axis(w.h, w.vh);
        if (tables.cubic && std::max(x.gain, y.gain) > PJD_BICUBIC_MAX_GAIN)
            return fault_of(spec, "the bicubic weights of %s sum to more than PJD_BICUBIC_MAX_GAIN in magnitude on an axis", i);
        out.aa[i] = PjdDevResizeAA{x.off, x.taps, y.off, y.taps};
        // the widest row segment one of its tiles stages: first tap of the tile's first column to the last tap of its last one
        for (uint32_t c0 = 0; c0 < r.tw; c0 += PJD_RS_COLS) {
            uint32_t e0, e1;                                // the tile's two ends in the table: mirrored where the window flips
            pjd_resize_win_ends(w, r.tw, c0, std::min(c0 + PJD_RS_COLS, r.tw) - 1u, e0, e1);
            const uint32_t h0 = out.tab[x.off + e0], h1 = out.tab[x.off + e1];
            form.lds = std::max(form.lds, pjd_resize_aa_lds((h1 & 0xffffu) + (h1 >> 16) - (h0 & 0xffffu), spec.planar, spec.channels));
        }
    }
    return blur_stage(spec, out);
}

PjdPackedLayout pjd_packed_layout(const uint32_t *w, const uint32_t *h, size_t n, uint64_t elem_bytes, uint32_t channels)
{
    PjdPackedLayout l;
    l.off.resize(n); l.bytes.resize(n);
    for (size_t i = 0; i < n; i++) {
        l.off[i] = l.buf_bytes; l.bytes[i] = (uint64_t)channels * w[i] * h[i] * elem_bytes;
        l.buf_bytes = (l.buf_bytes + l.bytes[i] + 255) & ~(uint64_t)255;
        l.sum += l.bytes[i];
    }
    return l;
}

uint32_t pjd_f32_to_dtype_bits(int dtype, float u)
{
    uint32_t bits;
    std::memcpy(&bits, &u, 4);
    if (dtype == PJD_DT_F32) return bits;
    if (dtype == PJD_DT_F16) return f32_to_f16_bits(u);
    bits += 0x7fffu + ((bits >> 16) & 1u);
    return bits >> 16;
}

PjdPadFill pjd_pad_fill(const PjdNormalize &norm, bool planar, const uint8_t fill[3], const float *pad_value)
{
    const uint32_t es = norm.dtype ? PJD_DT_SIZE(norm.dtype) : 1u;
    uint32_t e[3];
    for (int c = 0; c < 3; c++)
        e[c] = !norm.dtype ? fill[c] : pjd_f32_to_dtype_bits(norm.dtype, pad_value ? pad_value[c] : pjd_normalize_f32(fill[c], norm.scale[c], norm.bias[c]));
    PjdPadFill f{};
    uint8_t bytes[12];
    for (uint32_t t = 0; t < 12u; t++) bytes[t] = (uint8_t)(e[(t / es) % 3u] >> (8u * (t % es)));
    if (planar)
        for (int c = 0; c < 3; c++) f.d[c] = es == 1u ? e[c] * 0x01010101u : es == 2u ? e[c] * 0x00010001u : e[c];
    else
        std::memcpy(f.d, bytes, 12);
    return f;
}
