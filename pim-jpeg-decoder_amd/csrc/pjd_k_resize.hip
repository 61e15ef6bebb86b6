// pjd_k_resize.hip -- resize on decode (pjd_batch_set_resize): every picture of a ragged batch, as the back end left it at its decode
// size in the batch's intermediate buffer, resampled to its own target size in ONE launch.  The filter is the bilinear one
// include/pjd.h specifies bit for bit; its taps come from pjd_resize_tap_calc (pjd_internal.h), the function pjd_resize_tap exports.
//
// A memory-bound gather.  One wave takes one TILE of one picture (PJD_RS_ROWS target rows x PJD_RS_COLS target columns; the host's
// prefix sum over the pictures' tiles says which), a lane PJD_RS_PX = 4 adjacent pixels of each of its rows:
//   - the column taps (the divisions) are computed once per lane and serve all rows of the tile;
//   - the row taps are computed by the first PJD_RS_ROWS lanes, one row each, and read back as wave-uniform values;
//   - a lane's four pixels leave in one dword store per channel (planar) or three dwords (interleaved) where the address is
//     4-byte aligned and the row has four pixels left -- byte stores at a ragged right edge and for an unaligned destination
//     (pjd_batch_bind_output promises no alignment);
//   - the source is read with byte loads: the gather addresses of neighbouring lanes fall into the same or adjacent cache lines.
// Exactly the bytes of each picture's range are written, every one of them by every launch.
//
// Normalised float output (pjd_batch_set_normalize): the same taps and blends, and where the uint8 variant packs its four samples the
// float variants finish them -- one binary32 fma per sample (pjd_normalize_f32 of pjd_internal.h, the arithmetic include/pjd.h
// specifies), one conversion for the 16-bit types -- and store elements of 2 or 4 bytes: a lane's four pixels of one channel in one
// 8-byte (fp16 / bf16) or 16-byte (fp32) store planar, 24 or 48 bytes interleaved, where the address has that store's alignment and
// the row has four pixels left; element stores otherwise (pjd_batch_bind_output promises element alignment, no more).  The six
// constants are launch arguments: wave-uniform, they never pass through the per-picture record.
//
// The antialiased filter (pjd_batch_set_resize_filter, PJD_RESIZE_ANTIALIAS): the same launch -- the same tiles and prefix sum, a lane the
// same four pixels of each row of its tile -- with the widened triangle filter include/pjd.h specifies bit for bit.  A workgroup is ONE
// wave there: its barriers cost nothing.  An output sample has up to 32 x 32 taps, so nothing is gathered.  The filter is separable; a
// wave STREAMS down the source rows its tile reads, and for each of them
//   - stages the row's segment -- the source columns the tile's 256 target columns read -- in LDS with coalesced dword loads;
//   - filters it horizontally, once per tile and not once per target row: per lane 4 pixels x 3 channels, the taps as byte reads from
//     LDS (neighbouring lanes share most of them), the weights from the batch's table (tap-major: adjacent lanes, adjacent words;
//     padded with weight 0 up to the axis' largest count, so the loop bound is uniform) -> twelve h16;
//   - adds w * h16 to the accumulators of those of the tile's 8 target rows that have this source row among their taps -- a
//     wave-uniform test, the weight a scalar load.  8 x 12 accumulators live in registers (no scratch).
// Then the same epilogue.  The weights are made on the host (pjd_resize_aa_taps_calc, pjd_internal.h): no division here.
//
// The bicubic filter (PJD_RESIZE_BICUBIC): that launch again -- the same streaming, staging, tables (tap-major, now up to 64 taps an
// axis and weights of either sign) and epilogue -- with the signed arithmetic include/pjd.h specifies: signed 24-bit multiplies, the
// row sample with 6 fraction bits, one clamp at the end.  The body is the antialiased one with a compile-time FILT.
//
// Source windows (pjd_batch_set_resize_window): any filter from a WINDOW of the decoded picture to a window of a virtual target,
// mirrored left-right where asked -- flip(resize(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]) of include/pjd.h.  No arithmetic of
// its own: the taps are the same functions and tables with a shifted index, read from a per-picture record of its own
// (PjdDevResizeWin) beside PjdDevResize.  The gather and the table-driven filters are ONE body text each (pjd_k_resize_body.h, pjd_k_resize_aa_body.h) with a
// compile-time WIN: a batch without windows runs kernels built with the identity window, which are the kernels it ran before.
//
// Orientation (pjd_batch_set_orientation): the eight EXIF orientations, per picture, in that launch.  No arithmetic of its own either: the
// resample happens in the stored picture's coordinates and its result is permuted on the way out -- the left-right mirror is the
// tap mirror of the windows, the top-bottom one a mirrored store row, the transpose a second form of the epilogue (store_cols of
// pjd_k_resize_store.h) that stores a lane's eight rows of one column as eight adjacent samples.  The same bodies with a compile-time
// ORI, in kernels of their own (pjd_k_resize_ori, pjd_k_resize_ori_tab).
//
// Pad on decode (pjd_batch_set_resize_pad): the picture is a rectangle of a larger canvas.  The same bodies with a compile-time PAD, in
// kernels of their own again (pjd_k_resize_pad, pjd_k_resize_pad_tab): tiles, taps and mirrors are the content's, the stores' row
// length, plane and origin the canvas's.  The border is a second, small kernel's (pjd_k_resize_border): the two write disjoint bytes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/pjd.h"
#include "pjd_kernels.h"

namespace {

#include "pjd_k_resize_store.h"

template <bool PLANAR>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
             const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles)
{
    constexpr int DT = 0;
    constexpr bool WIN = false, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    const PjdDevResizeWin *const win = nullptr;
    const NormArgs nz{};
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_norm(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                  const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
    constexpr bool WIN = false, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    const PjdDevResizeWin *const win = nullptr;
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_win(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                 const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                 const NormArgs nz)
{
    constexpr bool WIN = true, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_aa(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa,
                const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];                      // one source row's segment (three plane segments where PLANAR)
    constexpr bool WIN = false, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    constexpr int FILT = PJD_RESIZE_ANTIALIAS;
    const PjdDevResizeWin *const win = nullptr;
#include "pjd_k_resize_aa_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_win_aa(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                    const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                    const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = true, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    constexpr int FILT = PJD_RESIZE_ANTIALIAS;
#include "pjd_k_resize_aa_body.h"
}

// the bicubic filter: the same two kernels with the body's other arithmetic
template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_cubic(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                   const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa,
                   const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = false, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    constexpr int FILT = PJD_RESIZE_BICUBIC;
    const PjdDevResizeWin *const win = nullptr;
#include "pjd_k_resize_aa_body.h"
}

template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64)
pjd_k_resize_win_cubic(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                       const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                       const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = true, ORI = false, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
    constexpr int FILT = PJD_RESIZE_BICUBIC;
#include "pjd_k_resize_aa_body.h"
}

// orientation (pjd_batch_set_orientation): the windowed kernels again, with the store side that reads the picture's orientation
// (PJD_RWI_* in the flags of its window record).  Kernels of their own and not a run-time branch of the windowed ones: a batch
// without an orientation launches exactly what it launched before (profiles/orientation.md).
template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_ori(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                 const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                 const NormArgs nz)
{
    constexpr bool WIN = true, ORI = true, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT, int FILT>
__global__ void __launch_bounds__(64)
pjd_k_resize_ori_tab(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                     const PjdDevResizeWin *__restrict__ win, const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles,
                     const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = true, ORI = true, PAD = false;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
    const PjdDevResizePad *const pad = nullptr;
#include "pjd_k_resize_aa_body.h"
}

// pad on decode (pjd_batch_set_resize_pad): the oriented kernels -- the most general form -- again, storing into a rectangle of a canvas:
// row length, plane and origin of the stores from the picture's PjdDevResizePad.  Kernels of their own for the reason the oriented
// ones are: a batch without a pad launches exactly what it launched before (profiles/resize_pad.md).
template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_pad(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                 const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const uint32_t *__restrict__ tile_prefix,
                 uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
    constexpr bool WIN = true, ORI = true, PAD = true;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT, int FILT>
__global__ void __launch_bounds__(64)
pjd_k_resize_pad_tab(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                     const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const uint32_t *__restrict__ tile_prefix,
                     uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes,
                     const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = true, ORI = true, PAD = true;
    constexpr int NC = 3;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
#include "pjd_k_resize_aa_body.h"
}

// A grey batch (PJD_OUT_GRAY8): one plane.  Routed through the most general form alone -- the padded kernels, with the identity window,
// orientation 1 and an all-zero pad where the batch asked for none -- so that one channel costs twelve instantiations and not sixty
// (profiles/gray_output.md).  The same bodies with NC = 1: the channel loops run once, the LDS row segment is one plane segment.
// Kernels of their own: the three-channel ones keep their symbols, code and registers.
template <int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_gray(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                  const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const uint32_t *__restrict__ tile_prefix,
                  uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
    constexpr bool PLANAR = true, WIN = true, ORI = true, PAD = true;
    constexpr int NC = 1;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
#include "pjd_k_resize_body.h"
}

template <int DT, int FILT>
__global__ void __launch_bounds__(64)
pjd_k_resize_gray_tab(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                      const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const uint32_t *__restrict__ tile_prefix,
                      uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa, const uint32_t *__restrict__ tab, uint32_t lds_bytes,
                      const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool PLANAR = true, WIN = true, ORI = true, PAD = true;
    constexpr int NC = 1;
    constexpr bool COL = false;
    const PjdDevColour *const colour = nullptr;
#include "pjd_k_resize_aa_body.h"
}

// A colour map (pjd_batch_set_colour): every output's 8-bit triple through a 3 x 4 map of its own, between the blend and the store
// (colour_px of pjd_k_resize_store.h; normative in include/pjd.h).  A lane holds all three channels of its pixels in registers at that
// point, so the map needs no LDS, no pass of its own and no change to either epilogue.  Routed through the most general form alone, as
// a grey batch is and for the same reason: 8 + 16 instantiations, not sixty more.  The same bodies with COL; kernels of their own, so
// that a batch without a colour map launches exactly what it launched before (profiles/colour_matrix.md).
template <bool PLANAR, int DT>
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_col(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                 const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const PjdDevColour *__restrict__ colour,
                 const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const NormArgs nz)
{
    constexpr bool WIN = true, ORI = true, PAD = true, COL = true;
    constexpr int NC = 3;
#include "pjd_k_resize_body.h"
}

template <bool PLANAR, int DT, int FILT>
__global__ void __launch_bounds__(64)
pjd_k_resize_col_tab(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs,
                     const PjdDevResizeWin *__restrict__ win, const PjdDevResizePad *__restrict__ pad, const PjdDevColour *__restrict__ colour,
                     const uint32_t *__restrict__ tile_prefix, uint32_t n_images, uint32_t n_tiles, const PjdDevResizeAA *__restrict__ aa,
                     const uint32_t *__restrict__ tab, uint32_t lds_bytes, const NormArgs nz)
{
    extern __shared__ uint32_t seg[];
    constexpr bool WIN = true, ORI = true, PAD = true, COL = true;
    constexpr int NC = 3;
#include "pjd_k_resize_aa_body.h"
}

// The border of the padded pictures: everything of a canvas outside its content rectangle, which the resample leaves alone, set to the
// fill.  One wave per canvas LINE (a row of the interleaved picture; a row of one plane), found by the prefix sum over the pictures'
// lines (pictures without a pad have none).  A line of the top or bottom band is one run of fill, any other line two: left and right
// of the content.  Plain coalesced stores of a pattern made once on the host (PjdPadFill): dwords from the first 4-byte aligned address
// of a run on, bytes before it and behind the last whole dword (at most three each: pjd_batch_bind_output promises element alignment,
// no more).  No byte of the content rectangle is written, and no byte outside the canvas.
__global__ void __launch_bounds__(64 * PJD_RS_WAVES)
pjd_k_resize_border(uint8_t *__restrict__ dst, const PjdDevResize *__restrict__ recs, const PjdDevResizePad *__restrict__ pad,
                    const uint32_t *__restrict__ line_prefix, uint32_t n_images, uint32_t n_lines, uint32_t planar, uint32_t es, const PjdPadFill fill)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t line = __builtin_amdgcn_readfirstlane(blockIdx.x * PJD_RS_WAVES + (threadIdx.x >> 6));
#include "pjd_k_resize_border_body.h"
}

// f(planar, dtype) with both as compile-time constants: THE dtype x layout dispatch of the resample launch
template <class F>
void for_layout_and_dtype(bool planar, int dtype, F f)
{
    const auto with_layout = [&](auto P) {
        switch (dtype) {
        case 0:           f(P, std::integral_constant<int, 0>{});           break;
        case PJD_DT_F16:  f(P, std::integral_constant<int, PJD_DT_F16>{});  break;
        case PJD_DT_BF16: f(P, std::integral_constant<int, PJD_DT_BF16>{}); break;
        default:          f(P, std::integral_constant<int, PJD_DT_F32>{});  break;
        }
    };
    if (planar) with_layout(std::true_type{}); else with_layout(std::false_type{});
}

}  // namespace

void pjd_launch_resize(hipStream_t s, const PjdResizeLaunch &a)
{
    if (a.n_tiles == 0) return;
    NormArgs nz{};
    for (int c = 0; c < 3; c++) { nz.scale[c] = a.norm.scale[c]; nz.bias[c] = a.norm.bias[c]; }
    // bilinear: PJD_RS_WAVES tiles per workgroup, no LDS; the table-driven filters: a workgroup is one wave with its row segment in LDS
    const bool tabled = a.filter != PJD_RESIZE_BILINEAR;
    const dim3 grid(tabled ? a.n_tiles : (a.n_tiles + PJD_RS_WAVES - 1) / PJD_RS_WAVES), block(tabled ? 64 : 64 * PJD_RS_WAVES);
    for_layout_and_dtype(a.planar, a.norm.dtype, [&](auto P, auto D) {
        constexpr bool PL = decltype(P)::value;
        constexpr int DT = decltype(D)::value;
        if (a.channels == 1) {                             // a grey batch: planar, one plane, always with win and pad records
            if (a.filter == PJD_RESIZE_BICUBIC)
                hipLaunchKernelGGL((pjd_k_resize_gray_tab<DT, PJD_RESIZE_BICUBIC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
            else if (tabled)
                hipLaunchKernelGGL((pjd_k_resize_gray_tab<DT, PJD_RESIZE_ANTIALIAS>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
            else
                hipLaunchKernelGGL((pjd_k_resize_gray<DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, nz);
            return;
        }
        if (a.colour) {                                    // a coloured batch: three channels, always with win and pad records
            if (a.filter == PJD_RESIZE_BICUBIC)
                hipLaunchKernelGGL((pjd_k_resize_col_tab<PL, DT, PJD_RESIZE_BICUBIC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
            else if (tabled)
                hipLaunchKernelGGL((pjd_k_resize_col_tab<PL, DT, PJD_RESIZE_ANTIALIAS>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.colour, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
            else
                hipLaunchKernelGGL((pjd_k_resize_col<PL, DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.win, a.pad, a.colour, a.tile_prefix, a.n_images, a.n_tiles, nz);
            return;
        }
        if (a.pad && a.filter == PJD_RESIZE_BICUBIC)
            hipLaunchKernelGGL((pjd_k_resize_pad_tab<PL, DT, PJD_RESIZE_BICUBIC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.pad && tabled)
            hipLaunchKernelGGL((pjd_k_resize_pad_tab<PL, DT, PJD_RESIZE_ANTIALIAS>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.pad)
            hipLaunchKernelGGL((pjd_k_resize_pad<PL, DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.win, a.pad, a.tile_prefix, a.n_images, a.n_tiles, nz);
        else if (a.oriented && a.filter == PJD_RESIZE_BICUBIC)
            hipLaunchKernelGGL((pjd_k_resize_ori_tab<PL, DT, PJD_RESIZE_BICUBIC>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.oriented && tabled)
            hipLaunchKernelGGL((pjd_k_resize_ori_tab<PL, DT, PJD_RESIZE_ANTIALIAS>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.oriented)
            hipLaunchKernelGGL((pjd_k_resize_ori<PL, DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, nz);
        else if (a.filter == PJD_RESIZE_BICUBIC && a.win)
            hipLaunchKernelGGL((pjd_k_resize_win_cubic<PL, DT>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.filter == PJD_RESIZE_BICUBIC)
            hipLaunchKernelGGL((pjd_k_resize_cubic<PL, DT>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (tabled && a.win)
            hipLaunchKernelGGL((pjd_k_resize_win_aa<PL, DT>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (tabled)
            hipLaunchKernelGGL((pjd_k_resize_aa<PL, DT>), grid, block, a.lds_bytes, s, a.src, a.dst, a.recs, a.tile_prefix, a.n_images, a.n_tiles, a.aa, a.tab, a.lds_bytes, nz);
        else if (a.win)
            hipLaunchKernelGGL((pjd_k_resize_win<PL, DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.win, a.tile_prefix, a.n_images, a.n_tiles, nz);
        else if constexpr (DT == 0)
            hipLaunchKernelGGL(pjd_k_resize<PL>, grid, block, 0, s, a.src, a.dst, a.recs, a.tile_prefix, a.n_images, a.n_tiles);
        else
            hipLaunchKernelGGL((pjd_k_resize_norm<PL, DT>), grid, block, 0, s, a.src, a.dst, a.recs, a.tile_prefix, a.n_images, a.n_tiles, nz);
    });
}

void pjd_launch_resize_border(hipStream_t s, const PjdBorderLaunch &a)
{
    if (a.n_lines == 0) return;
    hipLaunchKernelGGL(pjd_k_resize_border, dim3((a.n_lines + PJD_RS_WAVES - 1) / PJD_RS_WAVES), dim3(64 * PJD_RS_WAVES), 0, s, a.dst, a.recs, a.pad, a.line_prefix,
                       a.n_images, a.n_lines, a.planar ? 1u : 0u, a.elem_bytes, a.fill);
}
