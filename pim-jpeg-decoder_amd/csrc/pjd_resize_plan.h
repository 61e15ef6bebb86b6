// pjd_resize_plan.h -- resize on decode, host side: what a batch was asked for -> the work list of the resample launch.
//
// The records the kernels of pjd_k_resize.hip read are a PURE FUNCTION of the request: pjd_resize_resolve makes all of them from a
// PjdResizeSpec in one go, and every setter of pjd_api.hip (pjd_batch_set_resize, _set_resize_pad, _set_orientation,
// _set_resize_window, _set_resize_filter, _set_resize_affine, _set_colour, _set_blur) adds its argument to the batch's request and resolves again.  Each rule of include/pjd.h --
// content = canvas - pad, the transpose swap, window defaults, the mirror's exclusive-or, the prefix sums, the axis tables, the LDS of
// the launch, every limit -- is stated once, here.  Plain C++, no HIP: tools/resize_plan_host.cpp checks it on the CPU under the
// sanitizers, tools/resize_host.cpp runs the kernel bodies over its records.
#pragma once
#include <string>
#include <vector>

#include "../../include/pjd.h"
#include "pjd_internal.h"

// one inverse 2 x 3 map of pjd_batch_set_resize_affine, as given: {m00, m01, m02, m10, m11, m12}
struct PjdAffine { double m[6]; };

// one 3 x 4 colour map of pjd_batch_set_colour, as given: row-major, the last column in 8-bit levels
struct PjdColour { double m[12]; };

// What the caller said, nothing derived.  An optional array that was given (`*_set`) but is all neutral -- all-zero pads, orientations
// all 1, all-zero windows -- resolves to what its absence resolves to; the flags are what the call-order rules of the setters read.
struct PjdResizePicture {
    uint64_t src_off, dst_off;             // the picture at its decode size in the intermediate buffer; the delivered one in the result buffer
    uint32_t sw, sh, src_stride;           // decode size, and bytes per source row
};
struct PjdResizeSpec {
    std::vector<PjdResizePicture> pic;     // one per OUTPUT: entries may repeat a source and name sources in any order (pjd_batch_set_views)
    std::vector<uint32_t> view_pic;        // pjd_batch_set_views: the picture of every output (as many as `pic`); empty: output i is picture i.
                                           // Read by the fault texts alone ("view <v> (picture <p>)"): no record depends on it
    bool planar = false;
    uint32_t channels = 3;                 // 3, or 1 for a grey batch (PJD_OUT_GRAY8): planar with one plane; it always resolves to the padded form
    std::vector<uint32_t> out_w, out_h;    // pjd_batch_set_resize: the delivered canvases
    bool pad_set = false, ori_set = false, win_set = false, filter_set = false;
    std::vector<pjd_resize_pad> pad;       // pjd_batch_set_resize_pad, as given
    std::vector<uint8_t> orientation;      // pjd_batch_set_orientation, as given
    std::vector<pjd_resize_window> win;    // pjd_batch_set_resize_window, as given: zeros for defaults
    int filter = PJD_RESIZE_BILINEAR;      // pjd_batch_set_resize_filter
    // pjd_batch_set_resize_affine: an alternative to the per-axis request above, not a layer on it -- with affine_set none of pad_set,
    // ori_set, win_set and filter_set may be (pjd_resize_affine_excludes), in whichever order the two were asked for
    bool affine_set = false;
    std::vector<PjdAffine> affine;         // one inverse map per output, as given
    uint8_t affine_fill[3] = {0, 0, 0};    // what a tap outside the picture reads
    // pjd_batch_set_colour: a layer on either request.  It brings the most general per-axis form (as a grey batch does), or the warp form
    bool colour_set = false;
    std::vector<PjdColour> colour;         // one map per output, as given
    // pjd_batch_set_blur: a launch of its own behind either request (never with a pad).  The resample then writes U, uint8, into the blur
    // intermediate, and `pic[i].dst_off` -- the final range -- is where the blur record of output i writes
    bool blur_set = false;
    std::vector<pjd_blur> blur;            // one entry per output, as given
};

// What chooses the kernel and sizes its grid ...
struct PjdResizeForm {
    uint32_t tiles = 0, lines = 0, lds = 0;                     // tiles of the resample launch, canvas lines of the border launch, LDS bytes of a table-driven launch
    bool windowed = false, oriented = false, padded = false;    // the WIN / ORI / PAD kernels; padded implies oriented implies windowed
    bool warp = false;                                          // pjd_batch_set_resize_affine: the launch of pjd_k_warp.hip, whose tiles are PJD_WARP_COLS x PJD_WARP_ROWS; none of the three above
    bool coloured = false;                                      // pjd_batch_set_colour: the COL kernels; padded (so oriented and windowed), or warp
    bool blurred = false;                                       // pjd_batch_set_blur: the launch of pjd_k_blur.hip behind the resample or warp, which then writes the blur intermediate
    uint32_t blur_tiles = 0, blur_lds = 0;                      // ... its tiles (PJD_BLUR_COLS x PJD_BLUR_ROWS) and its LDS bytes: those of the batch's largest radius
    uint64_t blur_buf_bytes = 0;                                // ... and the intermediate: the packed layout of the uint8 outputs
};
// ... and everything it reads (pjd_internal.h).  win, pad + line_prefix, aa + tab are empty where the form does not read them.
struct PjdResizeWork {
    PjdResizeForm form;
    std::vector<PjdDevResize> recs;        // target: Q's content (the canvas less its pad, axes swapped where the orientation transposes)
    std::vector<uint32_t> tile_prefix;     // [n + 1]
    std::vector<PjdDevResizeWin> win;      // defaults resolved, flags: PJD_RW_HFLIP ^ pjd_orient_flags
    std::vector<PjdDevResizePad> pad;
    std::vector<uint32_t> line_prefix;     // [n + 1]
    std::vector<PjdDevResizeAA> aa;
    std::vector<uint32_t> tab;             // one axis table per distinct (source length, target length)
    std::vector<uint32_t> ct_w, ct_h;      // the content of each delivered picture: the canvas less its pad
    std::vector<PjdDevWarp> warp;          // form.warp: the quantised map of every output
    std::vector<PjdDevColour> colour;      // form.coloured: the quantised colour map of every output
    std::vector<PjdDevBlur> blur;          // form.blurred: one record per output (recs[i].dst_off is then its src_off, in the intermediate)
    std::vector<uint32_t> blur_prefix;     // [n + 1]: the tiles of the blur launch
    std::vector<uint32_t> blur_taps;       // row 0: {65536}; then one row per distinct (ksize, sigma) that is not the identity
};

// no fault: text is empty.  The text is what pjd_last_error reports behind the setter's own "set_...: "; picture -1: the batch as a whole,
// else the index of the output at fault (the view, where the batch has views)
struct PjdResizeFault {
    std::string text;
    int picture = -1;
    bool state = false;                    // the request is refused for what the batch took before (PJD_E_STATE), not for an argument (PJD_E_ARG)
};
// "picture <i>", or "view <i> (picture <p>)" where the request has views: how every fault text names an output
std::string pjd_resize_output_name(const PjdResizeSpec &spec, size_t i);
PjdResizeFault pjd_resize_resolve(const PjdResizeSpec &spec, PjdResizeWork &out);

// THE validation of a source window and of a pad record (include/pjd.h): null, or what is wrong with it
const char *pjd_resize_window_fault(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const pjd_resize_window *win, int filter);
const char *pjd_resize_pad_fault(uint32_t out_w, uint32_t out_h, const pjd_resize_pad *pad);

// THE rules of an affine map (include/pjd.h).  pjd_warp_quantise: m -> the Q40 record the kernels read, every coefficient
// llrint(m * 2^40) with the half pixels folded into b0 and b1; null, or what is wrong with m: a value that is not finite, a
// coefficient beyond the limits, which are checked on the quantised values.  pjd_resize_affine_fault: that, behind the sizes.
// pjd_resize_affine_excludes: null, or the setter among pad / orientation / window / filter that the request holds and an affine map
// excludes ("set_resize_pad", ...).
const char *pjd_warp_quantise(const double m[6], PjdDevWarp &out);
const char *pjd_resize_affine_fault(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const double m[6]);
const char *pjd_resize_affine_excludes(const PjdResizeSpec &spec);

// THE rules of a colour map (include/pjd.h), the one statement of its limits.  pjd_colour_quantise: m -> the Q16 record the kernels read,
// every value llrint(m * 65536), bit 0 of the flags set where that is the identity; null, or what is wrong with m: a value that is not
// finite, a weight beyond 16 or an offset beyond 4096 levels in magnitude, checked on the quantised values.
const char *pjd_colour_quantise(const double m[12], PjdDevColour &out);

// THE rules of a blur entry (include/pjd.h).  pjd_blur_fault: null, or what is wrong with it.  pjd_blur_taps_calc: the ksize taps of a
// checked entry with ksize > 0, the code pjd_blur_taps exports and the table of a batch is made with.
const char *pjd_blur_fault(const pjd_blur *blur);
void pjd_blur_taps_calc(uint32_t ksize, double sigma, uint32_t *q);

// The packed layout of a batch's results, as the planner lays out a batch's own buffer: n pictures of channels * w * h elements of
// elem_bytes at 256-byte aligned offsets
struct PjdPackedLayout {
    std::vector<uint64_t> off, bytes;
    uint64_t buf_bytes = 0, sum = 0;       // the buffer (what pjd_batch_packed_size reports); the pictures alone
};
PjdPackedLayout pjd_packed_layout(const uint32_t *w, const uint32_t *h, size_t n, uint64_t elem_bytes, uint32_t channels = 3);

// binary32 -> one element of a PJD_DT_* type in the low bytes of a word: ONE rounding to nearest even for the 16-bit types (the
// conversions of pjd_normalize_value, which the device makes in hardware)
uint32_t pjd_f32_to_dtype_bits(int dtype, float u);
// The fill as the border kernel takes it: the three elements -- the fill byte (norm.dtype 0), or its normalised value, or pad_value
// (null: none) converted once -- laid out over twelve bytes of a row
PjdPadFill pjd_pad_fill(const PjdNormalize &norm, bool planar, const uint8_t fill[3], const float *pad_value);
