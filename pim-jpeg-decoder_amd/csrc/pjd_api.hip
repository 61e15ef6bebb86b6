// pjd_api.hip -- the C ABI of include/pjd.h on top of the gfx950 kernels.
//
// Host-side flow of one batch (what replaces the reference's consumer thread,
// reference src/decoder_host.cpp:213-350):
//   create   plan (pjd_plan.cpp) + allocate HBM and pinned staging
//   upload   one packed H2D copy of the bitstreams + the small work lists
//   decode   table build -> lane words -> parallel Huffman decode (lane streams) -> DC scan over lanes -> fused
//            IDCT/colour; images routed to the exact kernel: dense scratch -> exact kernel -> dense IDCT/colour
//   sync     read the status words; any image the parallel decoder flagged is re-decoded by the
//            exact kernel (on the GPU) and its picture regenerated
//   download one D2H copy per picture
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pjd.h"
#include "pjd_kernels.h"
#include "pjd_libjpeg.h"
#include "pjd_lut_build.h"
#include "pjd_plan.h"
#include "pjd_resize_plan.h"

// Buffers of destroyed batches are kept per context and handed to the next batch (a steady stream of
// batches then allocates nothing); bounded by pool_cap, freed at pjd_close.
struct PoolBlock { void *p; size_t bytes; };
struct Pool {
    std::mutex m;                          // the owner takes and gives; any context of the device may flush (out of memory)
    std::vector<PoolBlock> free_blocks;
    size_t bytes = 0;
    void *take(size_t want, size_t &got)
    {
        std::lock_guard<std::mutex> l(m);
        int best = -1;
        for (size_t k = 0; k < free_blocks.size(); k++) {
            const size_t sz = free_blocks[k].bytes;
            if (sz >= want && sz <= 2 * want + (1u << 20) && (best < 0 || sz < free_blocks[best].bytes)) best = (int)k;
        }
        if (best < 0) return nullptr;
        void *p = free_blocks[best].p;
        got = free_blocks[best].bytes;
        bytes -= got;
        free_blocks.erase(free_blocks.begin() + best);
        return p;
    }
    bool give(void *p, size_t sz, size_t cap)
    {
        std::lock_guard<std::mutex> l(m);
        if (bytes + sz > cap) return false;
        free_blocks.push_back({p, sz}); bytes += sz;
        return true;
    }
    template <class F> void flush(F release)            // hand everything cached back to the runtime
    {
        std::lock_guard<std::mutex> l(m);
        for (PoolBlock &k : free_blocks) release(k.p);
        free_blocks.clear(); bytes = 0;
    }
};

struct pjd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Pool dev_pool, pin_pool;
    size_t pool_cap = (size_t)64 << 30;   // bytes of HBM kept for reuse (PJD_POOL_GB)
    std::string err;
    bool force_sequential = false;
    uint32_t sub_bytes_override = 0;
    int plan_mode = PJD_PLAN_LATENCY;     // pjd_set_plan_mode
    int poison = -1;                      // PJD_DEBUG_POISON: 0..255, the byte every allocation made for this context is filled with; -1: off
    // picture groups: the chains of groups 1.. run on these, forked from / joined to `stream` (created on first use)
    std::vector<hipStream_t> group_streams;
    std::vector<hipEvent_t> join_ev;
    hipEvent_t fork_ev = nullptr, tables_ev = nullptr;
};

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return PJD_E_HIP;                                                                   \
        }                                                                                       \
    } while (0)

namespace {

// Decodes issued and not yet drained, per device, over all contexts of the process.  A decode issued while the device has nothing else
// of ours to do spreads its picture groups over several streams (the back end of the light pictures then runs beside the last chains
// of the entropy decode: one batch alone finishes earlier); one issued while others run keeps to ONE stream -- several batches in
// flight fill the device by themselves, and more streams than the runtime has hardware queues serialise each other
// (measured: three groups 2.89 -> 2.59 ms for a batch alone, but 122 -> 91 GPix/s with four batches in flight).
std::atomic<int> g_active[64];

// every open context, so that a context that runs out of HBM can make the others of its device give their caches back
std::mutex g_ctx_m;
std::vector<pjd_ctx *> g_ctxs;

// PJD_DEBUG_POISON (a diagnostic switch, off unless set): device memory obtained for this context -- a fresh allocation or a block of
// the pool -- is filled with the byte on the context's stream before anything else touches it, page-locked memory with memset.  A
// kernel that reads a word its decode has not written then reads the poison instead of the zeros of fresh memory or the valid words of
// a destroyed batch (tests/test_gpu_poisoned_memory.py).  Never reached inside a stream capture: every allocation is
// made before the upload or after the stream has drained.
hipError_t poison_dev(pjd_ctx *ctx, void *p, size_t bytes)
{
    if (ctx->poison < 0 || !p || bytes == 0) return hipSuccess;
    return hipMemsetAsync(p, ctx->poison, bytes, ctx->stream);
}

int pool_dev_alloc(pjd_ctx *ctx, void **out, size_t bytes, std::vector<PoolBlock> &owned)
{
    if (bytes == 0) bytes = 16;
    size_t got = 0;
    void *p = ctx->dev_pool.take(bytes, got);
    if (!p) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {                                                // cached memory of every context on this device goes back; retry
            (void)hipGetLastError();
            std::lock_guard<std::mutex> l(g_ctx_m);
            for (pjd_ctx *c : g_ctxs)
                if (c->device == ctx->device) c->dev_pool.flush([](void *q) { (void)hipFree(q); });
            e = hipMalloc(&p, bytes);
        }
        if (e != hipSuccess) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return PJD_E_NOMEM; }
        got = bytes;
    }
    owned.push_back({p, got});
    *out = p;
    if (poison_dev(ctx, p, got) != hipSuccess) { (void)hipGetLastError(); ctx->err = "PJD_DEBUG_POISON: hipMemsetAsync failed"; return PJD_E_HIP; }
    return PJD_OK;
}

std::string fmt_name(const char *f, const std::string &name)          // f has one %s: "picture <i>" or "view <v> (picture <p>)"
{
    char buf[240];
    std::snprintf(buf, sizeof buf, f, name.c_str());
    return buf;
}

int pool_pin_alloc(pjd_ctx *ctx, void **out, size_t bytes, std::vector<PoolBlock> &owned)
{
    if (bytes == 0) bytes = 16;
    size_t got = 0;
    void *p = ctx->pin_pool.take(bytes, got);
    if (!p) {
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { ctx->err = "hipHostMalloc failed"; return PJD_E_NOMEM; }
        got = bytes;
    }
    owned.push_back({p, got});
    *out = p;
    if (ctx->poison >= 0) std::memset(p, ctx->poison, got);
    return PJD_OK;
}

}  // namespace

struct pjd_batch {
    pjd_ctx *ctx = nullptr;
    PjdPlan plan;
    PjdBackForm back{};                  // the form of the plan's back end (pjd_kernels.h), set once by pjd_batch_create
    PjdDevBatch dev{};
    // device memory of the batch that `dev` does not name
    PjdDevIdctWg *d_iwgs_dense = nullptr;
    PjdDevIdctWg *d_iwgs_dense_std = nullptr, *d_cwgs_std = nullptr;   // PJD_F_LIBJPEG pictures: ranges of those on the dense path, work list of the colour launch
    uint8_t *d_planes = nullptr;         // ... and their component planes (null: the batch holds no such picture)
    uint32_t *d_seq_list = nullptr;      // images routed to the exact kernel up front ...
    uint64_t *d_seq_base = nullptr;      // ... and where each one's data units start in the dense scratch
    int32_t *d_status_init = nullptr;
    uint64_t *d_opstate = nullptr;       // wave_gen + wave_desc + ticket
    size_t opstate_bytes = 0;
    uint8_t *d_in = nullptr, *h_in = nullptr;   // the input blob (work lists + bitstreams) in HBM / page-locked memory
    size_t in_bytes = 0, images_off = 0;        // ... its size, and where the image records (dev.images) lie in it
    int32_t *h_status = nullptr;         // pinned
    unsigned long long *h_stats = nullptr;   // pinned, 16 words
    std::vector<uint32_t> seq_list;      // what d_seq_list holds
    std::vector<PoolBlock> dev_blocks, pin_blocks;   // everything this batch took from the context's pools
    uint64_t device_bytes = 0;
    bool uploaded = false, decoded = false, settled = false;
    int n_fallback = 0;
    float exact_fallback_ms = 0;
    uint32_t n_entropy_errors = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph_groups = nullptr;           // the same decode with the picture groups' chains as parallel branches (pjd_internal.h)
    hipGraphExec_t graph_exec_groups = nullptr;
    bool counted = false;                        // this batch's decode is counted in g_active[device]
    int chains = 0;                              // pjd_batch_decode_chains: the form the last decode was issued in (0: none yet)
    int graph_chains[2] = {0, 0};                // ... and the form each captured graph holds (graph_exec, graph_exec_groups)
    // pjd_batch_bind_output: dev.out is the caller's memory (never freed, zeroed or pooled here)
    bool bound = false, bound_offsets = false;   // bound_offsets: the caller chose the picture offsets (no packed download)
    uint64_t bound_capacity = 0;
    std::vector<uint64_t> packed_off;            // the packed layout of the results (256-byte aligned offsets), kept for a second bind
    // Where the RESULT of a decode lies -- what download, output_offset / _size, device_output and bind_output speak about -- as
    // opposed to where the back end writes (dev.out + PjdDevImage::out_off).  The two are one and the same (res_out == dev.out, the
    // planner's offsets and sizes) until pjd_batch_set_resize separates them: the back end then keeps writing dev.out, the batch's
    // own buffer at the planner's offsets (the intermediate), and the resample launch writes the pictures at their target sizes
    // into res_out -- a second buffer of the batch, or the caller's memory once bound.
    uint8_t *res_out = nullptr;
    std::vector<uint64_t> res_off, res_bytes;
    uint64_t res_buf_bytes = 0, res_out_bytes = 0;   // packed size (what pjd_batch_packed_size reports), sum of res_bytes
    bool resized = false;                        // pjd_batch_set_resize
    // pjd_batch_set_views: the OUTPUTS of the batch are views, view v a resample of picture view_pic[v].  Everything above that speaks
    // about results (res_off / res_bytes, packed_off, the records of the pairs below) has n_out() entries; status words, the planner's
    // lists and the intermediate stay per picture.  Without the call output i is picture i.
    bool viewed = false;
    std::vector<uint32_t> view_pic;
    size_t n_out() const { return viewed ? view_pic.size() : plan.images.size(); }
    uint32_t pic_of(size_t v) const { return viewed ? view_pic[v] : (uint32_t)v; }
    std::string out_name(size_t v) const
    {
        char buf[64];
        if (viewed) std::snprintf(buf, sizeof buf, "view %zu (picture %u)", v, view_pic[v]);
        else std::snprintf(buf, sizeof buf, "picture %zu", v);
        return buf;
    }
    // The resample (pjd_resize_plan.h): what the caller asked for so far, and what it resolves to.  Every setter adds its argument to
    // the request and resolves all of it again; the records lie in the page-locked halves of the pairs below, pjd_batch_upload sends them.
    PjdResizeSpec spec;
    PjdResizeForm form;
    struct Pair { uint8_t *h = nullptr, *d = nullptr; size_t bytes = 0; };   // page-locked / HBM, taken once (take_pair)
    Pair rs;                                     // PjdDevResize[n_out], then the prefix sum of tiles [n_out + 1]
    Pair win;                                    // form.windowed: PjdDevResizeWin[n_out]
    Pair pad;                                    // form.padded: PjdDevResizePad[n_out], then the prefix sum of their border lines [n_out + 1]
    Pair aa;                                     // a table-driven filter: PjdDevResizeAA[n_out], then the weight table
    Pair warp;                                   // form.warp (pjd_batch_set_resize_affine): PjdDevWarp[n_out]
    Pair col;                                    // form.coloured (pjd_batch_set_colour): PjdDevColour[n_out]
    // form.blurred (pjd_batch_set_blur): PjdDevBlur[n_out], the prefix sum of the blur launch's tiles [n_out + 1], then the tap table; and
    // the blur intermediate, U of every output as uint8 in the packed layout.  The resample (or warp) launch then writes THAT, not
    // normalised, and the blur launch behind it writes res_out: the final offsets are the blur records' (set_result_offsets).
    Pair blur;
    uint8_t *d_blur_buf = nullptr;
    uint8_t *resample_dst() const { return form.blurred ? d_blur_buf : res_out; }
    PjdNormalize resample_norm() const { return form.blurred ? PjdNormalize{} : norm; }
    PjdNormalize norm{};                         // pjd_batch_set_normalize: dtype != 0, the result holds elements of PJD_DT_SIZE(dtype) bytes
    uint8_t pad_fill[3] = {0, 0, 0};             // pjd_batch_set_resize_pad
    bool pad_value_set = false;                  // pjd_batch_set_pad_value
    float pad_value[3] = {0, 0, 0};

    // the resample launch of this batch, whatever its filter and form
    void launch_resize(hipStream_t s) const
    {
        const size_t n = n_out();                // the records' count: the kernels find a tile's record by it, whatever picture the record reads
        const bool planar = back.planes();
        pjd_launch_resize(s, PjdResizeLaunch{dev.out, resample_dst(), (const PjdDevResize *)rs.d, (const uint32_t *)(rs.d + n * sizeof(PjdDevResize)), (uint32_t)n, form.tiles, planar, resample_norm(),
                                             form.windowed ? (const PjdDevResizeWin *)win.d : nullptr, form.oriented, spec.filter,
                                             (const PjdDevResizeAA *)aa.d, aa.d ? (const uint32_t *)(aa.d + n * sizeof(PjdDevResizeAA)) : nullptr, form.lds,
                                             form.padded ? (const PjdDevResizePad *)pad.d : nullptr, spec.channels,
                                             form.coloured ? (const PjdDevColour *)col.d : nullptr});
    }
    // the affine warp of this batch (form.warp), in place of the two launches around it: it writes the fill too
    void launch_warp(hipStream_t s) const
    {
        const size_t n = n_out();
        const uint8_t *f = spec.affine_fill;
        pjd_launch_warp(s, PjdWarpLaunch{dev.out, resample_dst(), (const PjdDevResize *)rs.d, (const PjdDevWarp *)warp.d, (const uint32_t *)(rs.d + n * sizeof(PjdDevResize)), (uint32_t)n, form.tiles,
                                         back.planes(), resample_norm(), (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16), spec.channels,
                                         form.coloured ? (const PjdDevColour *)col.d : nullptr});
    }
    // the blur of this batch (form.blurred), behind either: from the blur intermediate to the final ranges, normalised where asked for
    void launch_blur(hipStream_t s) const
    {
        const size_t n = n_out();
        const uint8_t *prefix = blur.d + n * sizeof(PjdDevBlur);
        pjd_launch_blur(s, PjdBlurLaunch{d_blur_buf, res_out, (const PjdDevBlur *)blur.d, (const uint32_t *)prefix, (const uint32_t *)(prefix + (n + 1) * sizeof(uint32_t)), (uint32_t)n,
                                         form.blur_tiles, back.planes(), norm, spec.channels, form.blur_lds});
    }
    // ... and the border of its padded pictures, behind it: the two write disjoint bytes
    void launch_pad(hipStream_t s) const
    {
        const size_t n = n_out();
        const bool planar = back.planes();
        pjd_launch_resize_border(s, PjdBorderLaunch{res_out, (const PjdDevResize *)rs.d, (const PjdDevResizePad *)pad.d, (const uint32_t *)(pad.d + n * sizeof(PjdDevResizePad)), (uint32_t)n,
                                                    form.lines, planar, norm.dtype ? PJD_DT_SIZE(norm.dtype) : 1u, pjd_pad_fill(norm, planar, pad_fill, pad_value_set ? pad_value : nullptr), spec.channels});
    }
};

namespace {

// A page-locked and a device block of `bytes` for the batch, from the context's pools, counted in device_bytes.  Taken once: a pair the
// batch has already is kept.  What a failing call took stays with the batch until it is destroyed.
int take_pair(pjd_batch *b, pjd_batch::Pair &p, size_t bytes)
{
    if (p.d) return PJD_OK;
    int rc = p.h ? PJD_OK : pool_pin_alloc(b->ctx, (void **)&p.h, bytes, b->pin_blocks);
    if (rc == PJD_OK) rc = pool_dev_alloc(b->ctx, (void **)&p.d, bytes, b->dev_blocks);
    if (rc != PJD_OK) return rc;
    p.bytes = bytes;
    b->device_bytes += bytes;
    return PJD_OK;
}

// one of the batch's device blocks back to the context's pool, and `counted` bytes off device_bytes
void give_back(pjd_batch *b, void *p, uint64_t counted)
{
    pjd_ctx *ctx = b->ctx;
    for (size_t k = 0; k < b->dev_blocks.size(); k++)
        if (b->dev_blocks[k].p == p) {
            if (!ctx->dev_pool.give(b->dev_blocks[k].p, b->dev_blocks[k].bytes, ctx->pool_cap)) hipFree(b->dev_blocks[k].p);
            b->dev_blocks.erase(b->dev_blocks.begin() + (long)k);
            b->device_bytes -= counted;
            break;
        }
}

// records, and what follows them, into the page-locked half of their pair
template <class A, class B = uint32_t>
void put(const pjd_batch::Pair &p, const std::vector<A> &a, const std::vector<B> &behind = {})
{
    if (!a.empty()) std::memcpy(p.h, a.data(), a.size() * sizeof(A));
    if (!behind.empty()) std::memcpy(p.h + a.size() * sizeof(A), behind.data(), behind.size() * sizeof(B));
}

// `spec` resolved to `w`: takes the buffers the records need that the batch does not have yet, then commits request and records.
// Nothing of the batch changes where it fails (but for a block that stays with it until it is destroyed).
int commit_request(pjd_batch *b, PjdResizeSpec &spec, const PjdResizeWork &w)
{
    hipSetDevice(b->ctx->device);
    const size_t n = spec.pic.size();
    int rc = take_pair(b, b->rs, n * sizeof(PjdDevResize) + (n + 1) * sizeof(uint32_t));
    if (rc == PJD_OK && w.form.windowed) rc = take_pair(b, b->win, n * sizeof(PjdDevResizeWin));
    if (rc == PJD_OK && w.form.padded) rc = take_pair(b, b->pad, n * sizeof(PjdDevResizePad) + (n + 1) * sizeof(uint32_t));
    if (rc == PJD_OK && spec.filter != PJD_RESIZE_BILINEAR) rc = take_pair(b, b->aa, n * sizeof(PjdDevResizeAA) + w.tab.size() * sizeof(uint32_t));
    if (rc == PJD_OK && w.form.warp) rc = take_pair(b, b->warp, n * sizeof(PjdDevWarp));
    if (rc == PJD_OK && w.form.coloured) rc = take_pair(b, b->col, n * sizeof(PjdDevColour));
    if (rc == PJD_OK && w.form.blurred) rc = take_pair(b, b->blur, n * sizeof(PjdDevBlur) + (n + 1) * sizeof(uint32_t) + w.blur_taps.size() * sizeof(uint32_t));
    if (rc == PJD_OK && w.form.blurred && !b->d_blur_buf) {            // the blur intermediate, taken once as the pairs are
        rc = pool_dev_alloc(b->ctx, (void **)&b->d_blur_buf, (size_t)w.form.blur_buf_bytes, b->dev_blocks);
        if (rc == PJD_OK) b->device_bytes += w.form.blur_buf_bytes;
    }
    if (rc != PJD_OK) return rc;
    put(b->rs, w.recs, w.tile_prefix);
    if (w.form.windowed) put(b->win, w.win);
    if (w.form.padded) put(b->pad, w.pad, w.line_prefix);
    if (spec.filter != PJD_RESIZE_BILINEAR) put(b->aa, w.aa, w.tab);
    if (w.form.warp) put(b->warp, w.warp);
    if (w.form.coloured) put(b->col, w.colour);
    if (w.form.blurred) {
        put(b->blur, w.blur, w.blur_prefix);
        std::memcpy(b->blur.h + n * sizeof(PjdDevBlur) + (n + 1) * sizeof(uint32_t), w.blur_taps.data(), w.blur_taps.size() * sizeof(uint32_t));
    }
    b->spec = std::move(spec);
    b->form = w.form;
    return PJD_OK;
}

// what every setter behind pjd_batch_set_resize does with the batch's request once its own argument is in it
int apply_request(pjd_batch *b, PjdResizeSpec &spec, const char *setter)
{
    PjdResizeWork w;
    const PjdResizeFault f = pjd_resize_resolve(spec, w);
    if (!f.text.empty()) { b->ctx->err = std::string(setter) + ": " + f.text; return f.state ? PJD_E_STATE : PJD_E_ARG; }
    return commit_request(b, spec, w);
}

// the delivered pictures at other offsets of the result buffer (pjd_batch_set_normalize, pjd_batch_bind_output): request and records
void set_result_offsets(pjd_batch *b, const std::vector<uint64_t> &off)
{
    // a blurred batch (pjd_batch_set_blur): the blur launch writes the results, the resample keeps writing the blur intermediate
    if (b->form.blurred) {
        PjdDevBlur *recs = (PjdDevBlur *)b->blur.h;
        for (size_t i = 0; i < off.size(); i++) b->spec.pic[i].dst_off = recs[i].dst_off = off[i];
        return;
    }
    PjdDevResize *recs = (PjdDevResize *)b->rs.h;
    for (size_t i = 0; i < off.size(); i++) b->spec.pic[i].dst_off = recs[i].dst_off = off[i];
}

// The order of the calls that shape a batch (include/pjd.h, CALL ORDER): the stages, each passed at most once but for the
// last two.  A new setter is a row here, at its place.
enum Stage { ST_NONE = -1, ST_VIEWS, ST_RESIZE, ST_PAD, ST_ORIENTATION, ST_WINDOW, ST_FILTER, ST_AFFINE, ST_COLOUR, ST_BLUR, ST_NORMALIZE, ST_PAD_VALUE, ST_BIND, ST_UPLOAD, N_STAGES };
struct StageRule {
    const char *name;                          // the call, as the messages spell it
    bool (*passed)(const pjd_batch *);         // has the batch been through it?
    bool repeatable;
    Stage needs[2];                            // the stages the call comes too early without ...
    const char *missing;                       // ... and what a call that needs THIS stage says where it is missing ("": none needs it)
};
const StageRule STAGES[N_STAGES] = {
    {"set_views",         [](const pjd_batch *b) { return b->viewed; },          false, {ST_NONE, ST_NONE},     ""},
    {"set_resize",        [](const pjd_batch *b) { return b->resized; },         false, {ST_NONE, ST_NONE},     "no resize is set (pjd_batch_set_resize first)"},
    {"set_resize_pad",    [](const pjd_batch *b) { return b->spec.pad_set; },    false, {ST_RESIZE, ST_NONE},   "the batch has no pad (pjd_batch_set_resize_pad first)"},
    {"set_orientation",   [](const pjd_batch *b) { return b->spec.ori_set; },    false, {ST_RESIZE, ST_NONE},   ""},
    {"set_resize_window", [](const pjd_batch *b) { return b->spec.win_set; },    false, {ST_RESIZE, ST_NONE},   ""},
    {"set_resize_filter", [](const pjd_batch *b) { return b->spec.filter_set; }, false, {ST_RESIZE, ST_NONE},   ""},
    {"set_resize_affine", [](const pjd_batch *b) { return b->spec.affine_set; }, false, {ST_RESIZE, ST_NONE},   ""},
    {"set_colour",        [](const pjd_batch *b) { return b->spec.colour_set; }, false, {ST_RESIZE, ST_NONE},   ""},
    {"set_blur",          [](const pjd_batch *b) { return b->spec.blur_set; },   false, {ST_RESIZE, ST_NONE},   ""},
    {"set_normalize",     [](const pjd_batch *b) { return b->norm.dtype != 0; }, false, {ST_NONE, ST_NONE},     "the batch is not normalised (pjd_batch_set_normalize first)"},
    {"set_pad_value",     [](const pjd_batch *b) { return b->pad_value_set; },   false, {ST_PAD, ST_NORMALIZE}, ""},
    {"bind_output",       [](const pjd_batch *b) { return b->bound; },           true,  {ST_NONE, ST_NONE},     ""},
    {"upload",            [](const pjd_batch *b) { return b->uploaded; },        true,  {ST_NONE, ST_NONE},     ""},
};

int refuse(pjd_batch *b, const std::string &why) { b->ctx->err = why; return PJD_E_STATE; }

// May the call of stage `s` be made on the batch now?  Of several reasons why not, the first of: a stage it needs is missing, it was
// made before, the earliest stage behind it that the batch has passed.
int check_order(pjd_batch *b, Stage s)
{
    const StageRule &r = STAGES[s];
    const std::string call = r.name;
    for (Stage need : r.needs)
        if (need != ST_NONE && !STAGES[need].passed(b)) return refuse(b, call + ": " + STAGES[need].missing);
    if (!r.repeatable && r.passed(b)) return refuse(b, call + ": already set for this batch");
    // the one exception: set_normalize brings a resize (the identity) where the batch has none, and set_views names the call that was made
    if (s == ST_VIEWS && STAGES[ST_NORMALIZE].passed(b)) return refuse(b, call + " after set_normalize");
    for (int t = s + 1; t < N_STAGES; t++)
        if (STAGES[t].passed(b)) return refuse(b, call + " after " + STAGES[t].name);
    return PJD_OK;
}

// views without a resample: nothing can deliver them, so `call` (upload, decode, capture, bind_output) is refused
int check_views_resolved(pjd_batch *b, const char *call)
{
    if (!b->viewed || b->resized) return PJD_OK;
    return refuse(b, std::string(call) + ": the batch has views but no resample (pjd_batch_set_resize or pjd_batch_set_normalize first)");
}

// the environment's plan mode and subsequence size, as pjd_open and pjd_plan_info both read them
int env_plan_mode()
{
    const char *pm = std::getenv("PJD_PLAN_MODE");
    return pm && (pm[0] == 't' || pm[0] == '1') ? PJD_PLAN_THROUGHPUT : PJD_PLAN_LATENCY;
}

uint32_t env_sub_bytes()
{
    const char *sb = std::getenv("PJD_SUB_BYTES");
    return sb ? (uint32_t)std::atoi(sb) : 0;
}

}  // namespace

extern "C" {

int pjd_version(void) { return PJD_VERSION; }

int pjd_open(int device_ordinal, pjd_ctx **out)
{
    if (!out) return PJD_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n) return PJD_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return PJD_E_NODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PJD_E_NODEVICE;   // kernels are built for gfx950 only
    pjd_ctx *c = new pjd_ctx;
    c->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return PJD_E_HIP;
    }
    const char *fs = std::getenv("PJD_FORCE_SEQUENTIAL");
    c->force_sequential = fs && fs[0] == '1';
    const char *pg = std::getenv("PJD_POOL_GB");
    if (pg) c->pool_cap = (size_t)std::atoll(pg) << 30;
    c->sub_bytes_override = env_sub_bytes();
    if (const char *po = std::getenv("PJD_DEBUG_POISON")) {                  // a byte, decimal or 0x..; anything else leaves the switch off
        char *end = nullptr;
        const long v = std::strtol(po, &end, 0);
        if (end != po && *end == 0 && v >= 0 && v <= 255) c->poison = (int)v;
    }
    c->plan_mode = env_plan_mode();
    { std::lock_guard<std::mutex> l(g_ctx_m); g_ctxs.push_back(c); }
    *out = c;
    return PJD_OK;
}

int pjd_set_plan_mode(pjd_ctx *ctx, int mode)
{
    if (!ctx) return PJD_E_ARG;
    if (mode != PJD_PLAN_LATENCY && mode != PJD_PLAN_THROUGHPUT) { ctx->err = "unknown plan mode"; return PJD_E_ARG; }
    ctx->plan_mode = mode;
    return PJD_OK;
}

void pjd_close(pjd_ctx *ctx)
{
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> l(g_ctx_m);
        for (size_t k = 0; k < g_ctxs.size(); k++)
            if (g_ctxs[k] == ctx) { g_ctxs.erase(g_ctxs.begin() + k); break; }
    }
    hipSetDevice(ctx->device);
    if (ctx->stream) { hipStreamSynchronize(ctx->stream); hipStreamDestroy(ctx->stream); }
    for (hipStream_t st : ctx->group_streams) { hipStreamSynchronize(st); hipStreamDestroy(st); }
    for (hipEvent_t ev : ctx->join_ev) hipEventDestroy(ev);
    if (ctx->fork_ev) hipEventDestroy(ctx->fork_ev);
    if (ctx->tables_ev) hipEventDestroy(ctx->tables_ev);
    ctx->dev_pool.flush([](void *q) { (void)hipFree(q); });
    ctx->pin_pool.flush([](void *q) { (void)hipHostFree(q); });
    delete ctx;
}

const char *pjd_last_error(pjd_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

const char *pjd_status_string(int status)
{
    switch (status & 0xFF) {   // reference src/jpeg_scanner.cpp:471,475,481,491,501,507,513
        case PJD_ST_OK: return "";
        case PJD_ST_DC_SYM: return "Error - Invalid DC value (255)";
        case PJD_ST_DC_LEN: return "Error - DC coefficient length greater than 11";
        case PJD_ST_DC_BITS: return "Error - Invalid DC value";
        case PJD_ST_AC_SYM: return "Error - Invalid AC value";
        case PJD_ST_AC_RUN: return "Error - Zero run-length exceeded block component";
        case PJD_ST_AC_LEN: return "Error - AC coefficient length greater than 10";
        case PJD_ST_AC_BITS: return "Error - Invalid AC value";
        default: return "Error - unknown";
    }
}

void *pjd_stream(pjd_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

void pjd_batch_destroy(pjd_batch *b)
{
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    if (b->counted) { g_active[b->ctx->device].fetch_sub(1); b->counted = false; }
    if (b->graph_exec) hipGraphExecDestroy(b->graph_exec);
    if (b->graph) hipGraphDestroy(b->graph);
    if (b->graph_exec_groups) hipGraphExecDestroy(b->graph_exec_groups);
    if (b->graph_groups) hipGraphDestroy(b->graph_groups);
    pjd_ctx *ctx = b->ctx;
    for (PoolBlock &k : b->dev_blocks)
        if (!ctx->dev_pool.give(k.p, k.bytes, ctx->pool_cap)) hipFree(k.p);
    for (PoolBlock &k : b->pin_blocks)
        if (!ctx->pin_pool.give(k.p, k.bytes, ctx->pool_cap / 4)) hipHostFree(k.p);
    delete b;
}

int pjd_batch_create(pjd_ctx *ctx, const pjd_image_desc *images, int n_images, int out_format, pjd_batch **out)
{
    if (!ctx || !out) return PJD_E_ARG;
    *out = nullptr;
    pjd_batch *b = new pjd_batch;
    b->ctx = ctx;
    std::vector<pjd_image_desc> forced;
    if (ctx->force_sequential && images && n_images > 0) {
        // PJD_FORCE_SEQUENTIAL=1: every picture as if its descriptor carried PJD_F_FORCE_SEQUENTIAL (a shard cannot: it keeps its path)
        forced.assign(images, images + n_images);
        for (pjd_image_desc &d : forced) if (d.shard_n_segs == 0) d.flags |= PJD_F_FORCE_SEQUENTIAL;
        images = forced.data();
    }
    int rc = pjd_make_plan(images, n_images, out_format, b->plan, ctx->err, ctx->sub_bytes_override, ctx->plan_mode);
    if (rc != PJD_OK) { delete b; return rc; }
    PjdPlan &P = b->plan;
    hipSetDevice(ctx->device);

    // One input blob per batch: the work lists and tables, then the packed bitstreams.  It is assembled in page-locked
    // memory now (the caller's buffers can go away) and goes up in ONE copy: every separate copy of a pageable vector is
    // staged by the runtime and waits its turn behind other streams' transfers on the copy engine (profiles/r02_pcie.md).
    auto fail = [&](int code) { pjd_batch_destroy(b); return code; };
    b->seq_list = P.seq_images;
    b->back = PjdBackForm{P.gray ? PJD_BACK_GRAY : (P.planar ? PJD_BACK_PLANAR : PJD_BACK_INTERLEAVED), P.scaled};
    std::vector<uint64_t> seq_base;
    std::vector<int32_t> st0(P.images.size(), 0);
    for (uint32_t i : b->seq_list) { st0[i] = PJD_STW_NEEDS_EXACT; seq_base.push_back(P.images[i].dense_base); }
    struct Part { const void *src; size_t bytes, off; void *dev; };        // dev: the batch's pointer to the part in HBM, set once d_in is known
    std::vector<Part> parts;
    size_t in_bytes = 0;
    auto part = [&](const auto &vec, size_t min_count, auto *&dev) {
        using T = std::remove_cv_t<std::remove_reference_t<decltype(vec[0])>>;
        static_assert(std::is_same<T, std::remove_cv_t<std::remove_reference_t<decltype(*dev)>>>::value, "the list and its device pointer differ in type");
        const size_t off = in_bytes;
        parts.push_back({vec.data(), vec.size() * sizeof(T), off, &dev});
        in_bytes = (off + std::max(vec.size(), std::max(min_count, (size_t)1)) * sizeof(T) + 255) & ~(size_t)255;
        return off;
    };
    b->images_off = part(P.images, 0, b->dev.images);
    part(P.tsets, 0, b->dev.tsets); part(P.tables, 0, b->dev.raw_tables); part(P.qtab, 0, b->dev.qtab); part(P.segs, 0, b->dev.segs); part(P.subs, 0, b->dev.lanes);
    part(P.hwaves, 0, b->dev.hwaves); part(P.hwgs, 0, b->dev.hwgs); part(P.iwgs, 0, b->dev.iwgs); part(P.iwgs_dense, 0, b->d_iwgs_dense); part(P.pscans, 0, b->dev.pscans);
    part(P.group_images, 0, b->dev.group_images); part(P.iwg_order, 0, b->dev.iwg_order);
    if (P.libjpeg) { part(P.iwgs_dense_std, 0, b->d_iwgs_dense_std); part(P.cwgs_std, 0, b->d_cwgs_std); }
    part(b->seq_list, (size_t)n_images, b->d_seq_list); part(seq_base, (size_t)n_images, b->d_seq_base); part(st0, (size_t)n_images, b->d_status_init);
    const size_t o_ecs = in_bytes;
    in_bytes += P.ecs_buf_bytes;
    b->in_bytes = in_bytes;
    if (pool_pin_alloc(ctx, (void **)&b->h_in, in_bytes, b->pin_blocks) != PJD_OK) return fail(PJD_E_NOMEM);
    for (const Part &q : parts) if (q.bytes) std::memcpy(b->h_in + q.off, q.src, q.bytes);
    {   // streams at their offsets, zeros in between (every stream is followed by >= 48 zero bytes)
        uint8_t *h_ecs = b->h_in + o_ecs;
        uint64_t pos = 0;
        for (int i = 0; i < n_images; i++) {
            const uint64_t off = P.images[i].ecs_off, len = P.host[i].ecs_copy_len;
            if (off > pos) std::memset(h_ecs + pos, 0, off - pos);
            if (len) std::memcpy(h_ecs + off, P.host[i].ecs_src, len);
            pos = off + len;
            if (P.images[i].flags & PJD_IF_PROGRESSIVE)              // its scans follow, each at its own offset
                for (uint32_t k = 0; k < P.images[i].n_pscan; k++) {
                    const PjdHostScan &hs = P.host_scans[P.images[i].pscan_base + k];
                    if (hs.off > pos) std::memset(h_ecs + pos, 0, hs.off - pos);
                    if (hs.len) std::memcpy(h_ecs + hs.off, hs.src, hs.len);
                    pos = hs.off + hs.len;
                }
        }
        std::memset(h_ecs + pos, 0, P.ecs_buf_bytes - pos);
    }
    if (pool_pin_alloc(ctx, (void **)&b->h_status, sizeof(int32_t) * (n_images + 1), b->pin_blocks) != PJD_OK) return fail(PJD_E_NOMEM);
    if (pool_pin_alloc(ctx, (void **)&b->h_stats, 16 * sizeof(unsigned long long), b->pin_blocks) != PJD_OK) return fail(PJD_E_NOMEM);

#define TRY_RC(x) do { int rc_ = (x); if (rc_ != PJD_OK) return fail(rc_); } while (0)
    auto dev_alloc = [&](auto *&dptr, size_t n) {                  // n elements from the context's pool, counted in device_bytes
        using T = std::remove_reference_t<decltype(*dptr)>;
        if (n == 0) n = 1;
        void *p = nullptr;
        const int r = pool_dev_alloc(ctx, &p, n * sizeof(T), b->dev_blocks);
        dptr = (T *)p;
        b->device_bytes += n * sizeof(T);
        return r;
    };
    const size_t n_hwave = P.hwaves.size();
    TRY_RC(dev_alloc(b->d_in, in_bytes));
    for (const Part &q : parts) { const uint8_t *p = b->d_in + q.off; std::memcpy(q.dev, &p, sizeof p); }      // every object pointer has this representation
    b->dev.ecs = b->d_in + o_ecs;
    if (P.libjpeg && !P.gray) TRY_RC(dev_alloc(b->d_planes, (size_t)P.plane_bytes));     // a grey batch has no component planes
    TRY_RC(dev_alloc(b->dev.luts, (size_t)P.lut_buf_bytes));
    TRY_RC(dev_alloc(b->dev.words, (size_t)P.n_words));
    TRY_RC(dev_alloc(b->dev.coef, P.dense_du * 64));
    TRY_RC(dev_alloc(b->dev.ent, (size_t)P.n_ent));
    TRY_RC(dev_alloc(b->dev.lane_info, P.subs.size()));
    TRY_RC(dev_alloc(b->dev.lane_dc, P.subs.size()));
    TRY_RC(dev_alloc(b->dev.dc_blk, (size_t)P.n_dcblk * 8));
    TRY_RC(dev_alloc(b->dev.marks, P.iwgs.size()));
    TRY_RC(dev_alloc(b->dev.out, P.out_buf_bytes));
    TRY_RC(dev_alloc(b->dev.status, (size_t)n_images));
    TRY_RC(dev_alloc(b->dev.imstate, (size_t)n_images));
    // wave_gen [PJD_GENS][n_hwave], wave_desc [n_hwave] and the ticket live in one allocation, zeroed before every launch
    // ... and a ticket per picture group
    const size_t op_words = n_hwave * (PJD_GENS + 1) + 2 + PJD_MAX_GROUPS;      // 64-bit words
    TRY_RC(dev_alloc(b->d_opstate, op_words));
    b->opstate_bytes = op_words * sizeof(uint64_t);
    b->dev.wave_gen = b->d_opstate;
    b->dev.wave_desc = b->d_opstate + n_hwave * PJD_GENS;
    b->dev.ticket = reinterpret_cast<uint32_t *>(b->d_opstate + n_hwave * (PJD_GENS + 1));
    if (std::getenv("PJD_DEBUG_STATS")) TRY_RC(dev_alloc(b->dev.dbg, n_hwave * 32));
    TRY_RC(dev_alloc(b->dev.stats, 16));
#undef TRY_RC
    b->dev.n_images = (uint32_t)n_images; b->dev.n_tsets = (uint32_t)P.tsets.size(); b->dev.n_lanes = (uint32_t)P.subs.size();
    b->dev.n_hwave = (uint32_t)n_hwave; b->dev.n_hwg = (uint32_t)P.hwgs.size();
    b->dev.n_iwg = (uint32_t)P.iwgs.size(); b->dev.n_dcblk = (uint32_t)P.n_dcblk;
    b->dev.sub_bytes = P.sub_bytes;
    b->dev.word_rows = PJD_WORD_ROWS(P.sub_bytes);
    b->dev.lane_cap = P.lane_cap;
    b->dev.max_lut_bytes = P.max_lut_bytes;
    b->res_out = b->dev.out;
    for (int i = 0; i < n_images; i++) { b->res_off.push_back(P.images[i].out_off); b->res_bytes.push_back(P.host[i].out_bytes); }
    b->res_buf_bytes = P.out_buf_bytes; b->res_out_bytes = P.out_bytes;
    *out = b;
    return PJD_OK;
}

int pjd_batch_upload(pjd_batch *b)
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (int rc = check_views_resolved(b, "upload")) return rc;
    hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    // asynchronous: the blob is page-locked and owned by the batch
    HIP_TRY(ctx, hipMemcpyAsync(b->d_in, b->h_in, b->in_bytes, hipMemcpyHostToDevice, s));
    // BMP row padding stays zero.  RGB8 and planar pictures are written whole by every decode, which is what a bound buffer
    // (pjd_batch_bind_output: the caller's memory, never BMP) relies on: it is not touched here.
    // With a resize set dev.out is the batch's intermediate, bound or not; the resized pictures are RGB8 or planar, written whole.
    if (!b->bound || b->resized) HIP_TRY(ctx, hipMemsetAsync(b->dev.out, 0, P.out_buf_bytes, s));
    if (b->resized) HIP_TRY(ctx, hipMemcpyAsync(b->rs.d, b->rs.h, b->rs.bytes, hipMemcpyHostToDevice, s));          // the resample work list (page-locked)
    if (b->aa.d) HIP_TRY(ctx, hipMemcpyAsync(b->aa.d, b->aa.h, b->aa.bytes, hipMemcpyHostToDevice, s));             // ... and its weight table
    if (b->form.windowed) HIP_TRY(ctx, hipMemcpyAsync(b->win.d, b->win.h, b->win.bytes, hipMemcpyHostToDevice, s));  // ... and its source windows
    if (b->form.padded) HIP_TRY(ctx, hipMemcpyAsync(b->pad.d, b->pad.h, b->pad.bytes, hipMemcpyHostToDevice, s));    // ... and its canvases
    if (b->form.warp) HIP_TRY(ctx, hipMemcpyAsync(b->warp.d, b->warp.h, b->warp.bytes, hipMemcpyHostToDevice, s));   // ... or its affine maps
    if (b->form.coloured) HIP_TRY(ctx, hipMemcpyAsync(b->col.d, b->col.h, b->col.bytes, hipMemcpyHostToDevice, s));  // ... and its colour maps
    if (b->form.blurred) HIP_TRY(ctx, hipMemcpyAsync(b->blur.d, b->blur.h, b->blur.bytes, hipMemcpyHostToDevice, s));  // ... and the work list and taps of its blur
    // What depends on the blob alone is made here, once per upload, behind its copy: the decode tables of every table set (the exact
    // path uses them too) and the lanes' word rows.  No kernel of a decode writes either, so every decode of
    // the resident batch -- launched or replayed from its graphs -- reads what this upload left.
    const bool parallel = !P.hwgs.empty();
    if (parallel || !b->seq_list.empty()) pjd_launch_build_tables(s, b->dev);
    if (parallel) pjd_launch_lane_words(s, b->dev);
    HIP_TRY(ctx, hipGetLastError());
    b->uploaded = true;
    return PJD_OK;
}

}  // extern "C"

// ---- the decode sequence -------------------------------------------------------------------
namespace {

struct KernelTimer {
    pjd_timings *t;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    std::vector<std::string> names;
    bool debug_sync = std::getenv("PJD_DEBUG_SYNC") != nullptr;
    void mark(const char *name)
    {
        if (debug_sync) {                                  // PJD_DEBUG_SYNC=1: name the launch a fault belongs to
            const hipError_t e = hipStreamSynchronize(s);
            std::fprintf(stderr, "[pjd] %-14s %s\n", name, e == hipSuccess ? "ok" : hipGetErrorString(e));
        }
        if (!t) return;
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, s);
        ev.push_back(e);
        names.push_back(name);
    }
    void finish()
    {
        if (!t) return;
        hipStreamSynchronize(s);
        t->n = 0;
        for (size_t k = 0; k + 1 < ev.size() && t->n < PJD_MAX_KERNELS; k++) {
            float ms = 0;
            hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            t->ms[t->n] = ms;
            std::snprintf(t->name[t->n], sizeof t->name[0], "%s", names[k + 1].c_str());
            t->n++;
        }
        t->total_ms = 0;
        if (ev.size() >= 2) hipEventElapsedTime(&t->total_ms, ev.front(), ev.back());
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
};

// streams and events for `ng` picture groups (group 0 uses the context's own stream)
bool ctx_group_streams(pjd_ctx *ctx, size_t ng)
{
    if (!ctx->fork_ev && hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming) != hipSuccess) { ctx->fork_ev = nullptr; return false; }
    if (!ctx->tables_ev && hipEventCreateWithFlags(&ctx->tables_ev, hipEventDisableTiming) != hipSuccess) { ctx->tables_ev = nullptr; return false; }
    while (ctx->group_streams.size() + 1 < ng) {
        hipStream_t st = nullptr;
        hipEvent_t ev = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { hipStreamDestroy(st); return false; }
        ctx->group_streams.push_back(st);
        ctx->join_ev.push_back(ev);
    }
    return true;
}

// Dense input: the ranges of the form's default kernel, then those of the PJD_F_LIBJPEG pictures (none: no launch) -- the exact path of
// a decode and the fallback of settle(), which brings a scratch (dv.coef) and lists of its own
void launch_dense(hipStream_t s, const pjd_batch *b, const PjdDevBatch &dv, const PjdDevIdctWg *wgs, size_t n, const PjdDevIdctWg *wgs_std, size_t n_std, size_t n_red,
                  const uint64_t *dense_base)
{
    pjd_launch_idct_dense(s, dv, b->back, wgs, dense_base, (uint32_t)n);
    pjd_launch_idct_std_dense(s, dv, b->back, wgs_std, dense_base, (uint32_t)n_std, (uint32_t)n_red, b->d_planes);     // n_std at full size, then n_red reduced
}

// Resize on decode: every picture from the intermediate (dev.out) to its target size in the result buffer, one launch, then the border
// of the padded pictures (a pad is set on a resize only).  kt: null, or the timed decode's marks.
void launch_resample(hipStream_t s, const pjd_batch *b, KernelTimer *kt)
{
    if (!b->resized) return;
    if (b->form.warp) {                                    // pjd_batch_set_resize_affine: the one launch, which writes the fill too
        b->launch_warp(s);
        if (kt) kt->mark("warp");
    } else {
        b->launch_resize(s);
        if (kt) kt->mark("resize");
        if (b->form.padded) {
            b->launch_pad(s);
            if (kt) kt->mark("pad");
        }
    }
    if (!b->form.blurred) return;
    b->launch_blur(s);                                     // pjd_batch_set_blur: what was just written is U, in the blur intermediate
    if (kt) kt->mark("blur");
}

int enqueue_decode(pjd_batch *b, pjd_timings *timings, bool use_groups)
{
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    hipStream_t s = ctx->stream;
    KernelTimer kt{timings, s, {}, {}};
    const bool parallel = !P.hwgs.empty();
    kt.mark("start");
    // One kernel of ours instead of two runtime memsets and a copy: status words from their initial values, statistics and
    // the words the Huffman waves publish to each other zeroed.  Inside a captured graph the runtime's small memset nodes are
    // not safe to replay next to other users of the runtime in the process: a 128-byte memset node replayed a 16-byte pattern
    // of stale pointers instead of zeros (seen with torch/gloo active before the capture; tools/r2 rehearsal of cfg5split).
    pjd_launch_reset(s, b->dev, b->d_status_init, parallel ? b->d_opstate : nullptr, parallel ? b->opstate_bytes / 8 : 0,
                     b->dev.dbg ? (uint32_t)(P.hwaves.size() * 32) : 0u);
    kt.mark("reset");
    // What a decode looks like on an otherwise idle device (use_groups), for a batch of many small pictures (the planner made groups):
    //   "groups" (default; any other word too) three chains of launches (pictures by density) on three streams
    //   "chain"  as with several batches in flight: one chain of launches
    static const bool idle_groups = [] { const char *e = std::getenv("PJD_IDLE_FORM"); return !e || std::strcmp(e, "chain") != 0; }();
    const bool idle = !timings && use_groups && parallel && !P.groups.empty() && idle_groups;       // per-kernel timing: one chain, kernel after kernel
    const PjdBackForm F = b->back;
    const size_t ng = idle ? P.groups.size() : 0;
    const bool grouped = ng > 1 && ctx_group_streams(ctx, ng);
    if (grouped) {
        // Picture groups (pjd_internal.h): every group's chain entropy decode -> DC predictors -> back end on a stream of its own,
        // forked from and joined to the context's stream with events (inside a stream capture these become parallel branches of the
        // graph).  Group 0 holds the densest pictures -- the longest chains of re-sync rounds -- and stays on the main stream.  The
        // chains have the same shape on purpose: with one branch a node longer than the other the graph ran the two entropy decodes
        // one after the other (4.65 ms instead of 2.60 for a batch alone; profiles/r04_experiments.md).
        HIP_TRY(ctx, hipEventRecord(ctx->fork_ev, s));
        for (size_t g = 0; g < ng; g++) {
            hipStream_t gs = g == 0 ? s : ctx->group_streams[g - 1];
            if (g) HIP_TRY(ctx, hipStreamWaitEvent(gs, ctx->fork_ev, 0));
            pjd_launch_huff_lanes_group(gs, b->dev, P.groups[g], (uint32_t)g);
            pjd_launch_group_dc(gs, b->dev, P.groups[g]);
            pjd_launch_idct_lanes(gs, b->dev, F, b->dev.iwg_order + P.groups[g].iwg_first, P.groups[g].iwg_count);
            if (g) { HIP_TRY(ctx, hipEventRecord(ctx->join_ev[g - 1], gs)); }
        }
        for (size_t g = 1; g < ng; g++) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->join_ev[g - 1], 0));
    } else {
        if (parallel) {
            pjd_launch_huff_lanes(s, b->dev);    kt.mark("huff_lanes");
            pjd_launch_lane_dc_scan(s, b->dev, P.dc_per_picture);  kt.mark("dc_scan");
            // a batch with PJD_F_LIBJPEG pictures: the ranges of the others come first in iwg_order and go through the form's default
            // kernel, those of the flagged ones into their planes (a grey batch: straight into the picture)
            pjd_launch_idct_lanes(s, b->dev, F, P.libjpeg ? b->dev.iwg_order : nullptr, P.libjpeg ? P.n_iwg_def : b->dev.n_iwg);
            kt.mark(F.gray() ? "idct_gray" : "idct_colour");
            if (P.n_iwg_std + P.n_iwg_red) {         // the reduced pictures' ranges (PJD_F_LIBJPEG_SCALE_*) stand behind: a launch of their own, one timed name
                pjd_launch_idct_std_lanes(s, b->dev, F, b->dev.iwg_order + P.n_iwg_def, P.n_iwg_std, P.n_iwg_red, b->d_planes);
                kt.mark(F.gray() ? "idct_gray_std" : "idct_std");
            }
        }
    }
    if (!b->seq_list.empty()) {
        // images routed to the exact kernel: dense int16 scratch, cleared first (unvisited slots are zero)
        pjd_launch_zero(s, b->dev.coef, P.dense_du * 64 * sizeof(int16_t));      // a kernel, not a memset node: see the reset above
        pjd_launch_huff_sequential(s, b->dev, b->d_seq_list, b->d_seq_base, (uint32_t)b->seq_list.size());
        if (!P.pscans.empty()) pjd_launch_progressive(s, b->dev, b->d_seq_list, b->d_seq_base, (uint32_t)b->seq_list.size());
        launch_dense(s, b, b->dev, b->d_iwgs_dense, P.iwgs_dense.size(), b->d_iwgs_dense_std, P.libjpeg ? P.n_dense_std : 0, P.libjpeg ? P.n_dense_red : 0, b->d_seq_base);
        kt.mark("exact_path");
    }
    if (P.libjpeg && !F.gray()) {
        // the flagged pictures' planes are complete, whichever front end filled them: upsample, colour, store
        pjd_launch_colour_std(s, b->dev, b->d_cwgs_std, P.n_cwg_std, P.n_cwg_red, b->d_planes);
        kt.mark("colour_std");
    }
    launch_resample(s, b, &kt);          // behind whatever form the back end took (the groups' streams have joined `s` above)
    HIP_TRY(ctx, hipGetLastError());
    kt.finish();
    b->decoded = true;
    b->settled = false;
    b->chains = grouped ? (int)ng : 1;           // what was issued, not what the planner made (pjd_batch_capture puts its own back)
    return PJD_OK;
}

// The temporary device blocks and events of one call: plain hipMalloc (rare paths with sizes of their own: never the context's pool),
// all of it released when the owner goes out of scope, whichever way the call ends.
struct Scratch {
    std::vector<void *> blocks;
    std::vector<hipEvent_t> events;
    bool out_of_memory = false;                  // an alloc() failed
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    ~Scratch() { for (hipEvent_t e : events) (void)hipEventDestroy(e); for (void *p : blocks) (void)hipFree(p); }
    template <class T> hipError_t alloc(T *&p, size_t bytes)
    {
        const hipError_t e = hipMalloc((void **)&p, bytes);
        if (e == hipSuccess) blocks.push_back(p); else { p = nullptr; out_of_memory = true; }
        return e;
    }
    hipEvent_t event()                           // null where the runtime gives none: the caller then does without
    {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) == hipSuccess) events.push_back(e); else e = nullptr;
        return e;
    }
};

// "Decode these pictures again with the exact kernel into a scratch of their own" (settle(), pjd_batch_download_coefficients).  list /
// base [n]: the pictures, and where each one's units start in a dense scratch of `du` units; extra: a further array that goes up with
// them (null: none); before: an event recorded in front of the exact kernel (null: none).  Enqueues the poison fills, the zero kernel,
// the copies and the exact kernel on `dv` (dev with coef = the scratch); d[]: scratch, list, base, extra on the device, owned by `tmp`.
hipError_t redo_exact(const pjd_batch *b, Scratch &tmp, const uint32_t *list, const uint64_t *base, size_t n, uint64_t du, const void *extra, size_t extra_bytes,
                      hipEvent_t before, PjdDevBatch &dv, uint8_t *d[4])
{
    hipStream_t s = b->ctx->stream;
    const void *h[4] = {nullptr, list, base, extra};
    const size_t bytes[4] = {(size_t)du * 64 * sizeof(int16_t), n * sizeof(uint32_t), n * sizeof(uint64_t), extra_bytes};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; k++) { d[k] = nullptr; if (k == 0 || h[k]) e = tmp.alloc(d[k], bytes[k]); }
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = poison_dev(b->ctx, d[k], bytes[k]);
    if (e != hipSuccess) return e;
    pjd_launch_zero(s, d[0], bytes[0]);          // our own kernel, as everywhere on the decode path
    e = hipGetLastError();
    for (int k = 1; k < 4 && e == hipSuccess; k++) if (h[k]) e = hipMemcpyAsync(d[k], h[k], bytes[k], hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    dv = b->dev;
    dv.coef = (int16_t *)d[0];
    if (before) (void)hipEventRecord(before, s);
    pjd_launch_huff_sequential(s, dv, (const uint32_t *)d[1], (const uint64_t *)d[2], (uint32_t)n);
    return hipSuccess;
}

// After the stream drained: re-decode, with the exact kernel, every image the parallel decoder
// flagged -- all of them in ONE launch, into a dense scratch allocated for just them (a rare path: corrupt
// or otherwise irregular streams).  Runs on the GPU.  A shard is re-decoded over its own segment range.
// As in the reference (decoder_host.cpp:181 drops decode_Huffman_data's result) such an image keeps its status
// and its partial picture; the rest of the batch is unaffected.
int settle(pjd_batch *b)
{
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    hipStream_t s = ctx->stream;
    if (b->settled || !b->decoded) return PJD_OK;
    const size_t n = P.images.size();
    HIP_TRY(ctx, hipMemcpyAsync(b->h_status, b->dev.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (b->counted) { g_active[ctx->device].fetch_sub(1); b->counted = false; }       // this decode has left the device
    std::vector<uint32_t> fb;
    std::vector<uint64_t> fb_base;
    std::vector<PjdDevIdctWg> fb_wgs, fb_wgs_std, fb_wgs_red;      // ranges to redo: of the default back end, of the PJD_F_LIBJPEG one at full size and reduced
    std::vector<char> was_seq(n, 0);
    for (uint32_t i : b->seq_list) was_seq[i] = 1;
    uint64_t du = 0;
    for (size_t i = 0; i < n; i++)
        if ((b->h_status[i] & PJD_STW_NEEDS_EXACT) && !was_seq[i]) {
            const PjdDevImage &g = P.images[i];
            for (uint32_t k = 0; k < g.n_iwg; k++) {
                PjdDevIdctWg w = P.iwgs[g.iwg_base + k];
                w.pad_ = (uint32_t)fb.size();
                ((g.flags & PJD_IF_LIBJPEG) ? ((g.flags & PJD_IF_LJSCALE_MASK) ? fb_wgs_red : fb_wgs_std) : fb_wgs).push_back(w);
            }
            fb.push_back((uint32_t)i);
            fb_base.push_back(du);
            du += (uint64_t)(g.last_mcu - g.first_mcu) * g.dus_per_mcu;
        }
    b->n_fallback = (int)fb.size();
    b->exact_fallback_ms = 0;
    b->n_entropy_errors = 0;
    for (size_t i = 0; i < n; i++)
        if (!(b->h_status[i] & PJD_STW_NEEDS_EXACT) && (b->h_status[i] & 0xFF) != 0) b->n_entropy_errors++;
    if (!fb.empty()) {
        const size_t n_def = fb_wgs.size(), n_std = fb_wgs_std.size(), n_red = fb_wgs_red.size();
        fb_wgs.insert(fb_wgs.end(), fb_wgs_std.begin(), fb_wgs_std.end());       // one list on the device: the default ranges, then the others
        fb_wgs.insert(fb_wgs.end(), fb_wgs_red.begin(), fb_wgs_red.end());
        Scratch tmp;
        hipEvent_t ev0 = tmp.event(), ev1 = tmp.event();          // exact_fallback_ms: from the exact kernel to the colour launch
        PjdDevBatch dv;
        uint8_t *d[4];                                            // the scratch, the list, the bases and the ranges on the device
        hipError_t e = redo_exact(b, tmp, fb.data(), fb_base.data(), fb.size(), du, fb_wgs.data(), fb_wgs.size() * sizeof(PjdDevIdctWg), ev0, dv, d);
        if (tmp.out_of_memory) { ctx->err = "hipMalloc failed for the exact-kernel scratch"; return PJD_E_NOMEM; }
        if (e == hipSuccess) {
            const PjdDevIdctWg *d_wgs = (const PjdDevIdctWg *)d[3];
            launch_dense(s, b, dv, d_wgs, n_def, d_wgs + n_def, n_std, n_red, (const uint64_t *)d[2]);
            // flagged pictures had their planes filled again: the colour launch (all flagged pictures of the batch: a rare path)
            if (n_std + n_red && !b->back.gray()) pjd_launch_colour_std(s, dv, b->d_cwgs_std, P.n_cwg_std, P.n_cwg_red, b->d_planes);
            if (ev1) (void)hipEventRecord(ev1, s);
            // the pictures just decoded again changed in the intermediate: resample (the whole batch: a rare path)
            launch_resample(s, b, nullptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(b->h_status, b->dev.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);        // also: the host vectors above are pageable
        if (e == hipSuccess && ev0 && ev1) (void)hipEventElapsedTime(&b->exact_fallback_ms, ev0, ev1);
        if (e != hipSuccess) { ctx->err = std::string("exact-kernel fallback: ") + hipGetErrorString(e); return PJD_E_HIP; }
    }
    b->settled = true;
    return PJD_OK;
}

}  // namespace

extern "C" {

static bool device_idle_then_count(pjd_batch *b)
{
    const int dev = b->ctx->device;
    if (dev < 0 || dev >= 64) return false;
    const int before = b->counted ? g_active[dev].load() - 1 : g_active[dev].fetch_add(1);
    b->counted = true;
    static const int force = [] { const char *e = std::getenv("PJD_GROUPS_ALWAYS"); return e ? std::atoi(e) : -1; }();   // experiments: 1 always, 0 never
    if (force >= 0) return force != 0;
    return before <= 0;
}

int pjd_batch_decode(pjd_batch *b)
{
    if (!b) return PJD_E_ARG;
    if (int rc = check_views_resolved(b, "decode")) return rc;
    if (!b->uploaded) { b->ctx->err = "decode before upload"; return PJD_E_STATE; }
    hipSetDevice(b->ctx->device);
    const bool groups = !b->plan.groups.empty() && device_idle_then_count(b);
    if (b->graph_exec) {
        hipGraphExec_t ge = (groups && b->graph_exec_groups) ? b->graph_exec_groups : b->graph_exec;
        HIP_TRY(b->ctx, hipGraphLaunch(ge, b->ctx->stream));
        b->decoded = true; b->settled = false;
        b->chains = b->graph_chains[ge == b->graph_exec ? 0 : 1];
        return PJD_OK;
    }
    return enqueue_decode(b, nullptr, groups);
}

int pjd_batch_decode_timed(pjd_batch *b, pjd_timings *t)
{
    if (!b || !t) return PJD_E_ARG;
    if (int rc = check_views_resolved(b, "decode")) return rc;          // the timed decode speaks as the decode
    if (!b->uploaded) { b->ctx->err = "decode before upload"; return PJD_E_STATE; }
    hipSetDevice(b->ctx->device);
    std::memset(t, 0, sizeof *t);
    return enqueue_decode(b, t, false);
}

int pjd_batch_capture(pjd_batch *b)
{
    if (!b) return PJD_E_ARG;
    if (int rc = check_views_resolved(b, "capture")) return rc;
    if (!b->uploaded) { b->ctx->err = "capture before upload"; return PJD_E_STATE; }
    pjd_ctx *ctx = b->ctx;
    hipSetDevice(ctx->device);
    if (b->graph_exec) return PJD_OK;
    for (int variant = 0; variant < (b->plan.groups.empty() ? 1 : 2); variant++) {
        // variant 0: the whole batch in one chain of launches; variant 1: the picture groups' chains as parallel branches
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        const int chains = b->chains;              // a capture is no decode: pjd_batch_decode_chains keeps speaking about the last one
        int rc = enqueue_decode(b, nullptr, variant == 1);
        b->graph_chains[variant] = b->chains;
        b->chains = chains;
        hipGraph_t &gr = variant ? b->graph_groups : b->graph;
        hipError_t e = hipStreamEndCapture(ctx->stream, &gr);
        b->decoded = false;
        if (rc != PJD_OK) return rc;
        if (e != hipSuccess) { ctx->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); return PJD_E_HIP; }
        HIP_TRY(ctx, hipGraphInstantiate(variant ? &b->graph_exec_groups : &b->graph_exec, gr, nullptr, nullptr, 0));
    }
    return PJD_OK;
}

int pjd_batch_decode_chains(pjd_batch *b)
{
    return b ? b->chains : PJD_E_ARG;
}

int pjd_batch_sync(pjd_batch *b)
{
    if (!b) return PJD_E_ARG;
    hipSetDevice(b->ctx->device);
    if (b->decoded) return settle(b);
    HIP_TRY(b->ctx, hipStreamSynchronize(b->ctx->stream));
    return PJD_OK;
}

int pjd_batch_download(pjd_batch *b, uint8_t *const *out, int32_t *status)
{
    if (!b) return PJD_E_ARG;
    if (!b->decoded) { b->ctx->err = "download before decode"; return PJD_E_STATE; }
    hipSetDevice(b->ctx->device);
    int rc = settle(b);
    if (rc != PJD_OK) return rc;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (out)
        for (size_t i = 0; i < b->n_out(); i++)                  // the outputs: the views where the batch has them; the status words stay per picture
            if (out[i]) HIP_TRY(ctx, hipMemcpyAsync(out[i], b->res_out + b->res_off[i], b->res_bytes[i], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (status)
        for (size_t i = 0; i < P.images.size(); i++) status[i] = b->h_status[i] & 0xFF;
    return PJD_OK;
}

int pjd_batch_download_packed(pjd_batch *b, uint8_t *host, uint64_t capacity, int32_t *status)
{
    if (!b || !host) return PJD_E_ARG;
    if (!b->decoded) { b->ctx->err = "download before decode"; return PJD_E_STATE; }
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    hipSetDevice(ctx->device);
    if (b->bound_offsets) { ctx->err = "download_packed: the batch is bound with explicit picture offsets (no packed layout)"; return PJD_E_STATE; }
    if (capacity < b->res_buf_bytes) { ctx->err = "download_packed: buffer smaller than pjd_batch_packed_size"; return PJD_E_ARG; }
    // a bound buffer need not reach past its last picture (the packed size is rounded up to 256 bytes)
    const uint64_t copy_bytes = b->bound && b->bound_capacity < b->res_buf_bytes ? b->bound_capacity : b->res_buf_bytes;
    int rc = settle(b);
    if (rc != PJD_OK) return rc;
    // the runtime's copy (SDMA engine): a copy kernel into mapped host memory lost to it, 9.1 against 11.8 GPix/s (profiles/r02_pcie.md)
    HIP_TRY(ctx, hipMemcpyAsync(host, b->res_out, copy_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (status)
        for (size_t i = 0; i < P.images.size(); i++) status[i] = b->h_status[i] & 0xFF;
    return PJD_OK;
}

uint64_t pjd_batch_packed_size(pjd_batch *b) { return b ? b->res_buf_bytes : 0; }

uint64_t pjd_batch_output_offset(pjd_batch *b, int image)
{
    if (!b || image < 0 || (size_t)image >= b->n_out()) return 0;
    return b->res_off[image];
}

int pjd_batch_bind_output(pjd_batch *b, void *device_base, uint64_t capacity, const uint64_t *offsets)
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (int rc = check_order(b, ST_BIND)) return rc;
    if (int rc = check_views_resolved(b, "bind_output")) return rc;
    if (!device_base) { ctx->err = "bind_output: null pointer"; return PJD_E_ARG; }
    if (P.out_format == PJD_OUT_BMP) { ctx->err = "bind_output: a BMP batch cannot be bound (its row padding relies on the batch's own zeroed buffer)"; return PJD_E_ARG; }
    hipSetDevice(ctx->device);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, device_base) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != ctx->device) {
        (void)hipGetLastError();
        ctx->err = "bind_output: not device memory of the context's device";
        return PJD_E_ARG;
    }
    {   // [base, base + capacity) lies inside the allocation the pointer belongs to (skipped where the runtime cannot tell; under a
        // sub-allocator such as torch's the allocation is its whole segment: this catches a wild capacity, no more)
        hipDeviceptr_t a_base = nullptr;
        size_t a_size = 0;
        if (hipMemGetAddressRange(&a_base, &a_size, (hipDeviceptr_t)device_base) != hipSuccess) (void)hipGetLastError();
        else if ((uintptr_t)device_base - (uintptr_t)a_base > a_size || capacity > a_size - ((uintptr_t)device_base - (uintptr_t)a_base)) {
            ctx->err = "bind_output: capacity reaches past the end of the allocation";
            return PJD_E_ARG;
        }
    }
    const size_t n = b->n_out();                                     // the outputs: pictures, or views
    if (b->packed_off.empty()) b->packed_off = b->res_off;
    std::vector<std::pair<uint64_t, uint64_t>> ranges(n);            // (offset, size) of every output
    for (size_t i = 0; i < n; i++) {
        ranges[i] = {offsets ? offsets[i] : b->packed_off[i], b->res_bytes[i]};
        if (ranges[i].first > capacity || ranges[i].second > capacity - ranges[i].first) { ctx->err = fmt_name("bind_output: %s ends beyond the capacity", b->out_name(i)); return PJD_E_ARG; }
        if (b->norm.dtype != 0 && ((uintptr_t)device_base + ranges[i].first) % PJD_DT_SIZE(b->norm.dtype) != 0) {
            ctx->err = fmt_name("bind_output: %s does not start at a multiple of the element size (pjd_batch_set_normalize)", b->out_name(i));
            return PJD_E_ARG;
        }
    }
    {
        std::vector<std::pair<uint64_t, uint64_t>> sorted = ranges;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 1; i < n; i++)
            if (sorted[i - 1].first + sorted[i - 1].second > sorted[i].first) { ctx->err = b->viewed ? "bind_output: view ranges overlap" : "bind_output: picture ranges overlap"; return PJD_E_ARG; }
    }
    // from here on nothing fails.  The batch's own result buffer goes back to the pool.  Without a resize the result is what the back
    // end writes: the planner's image records (and their copy in the input blob, which pjd_batch_upload sends) take the bound
    // offsets.  With one, only the resample's work list does: the back end keeps writing the intermediate at the planner's offsets.
    if (!b->bound) give_back(b, b->res_out, b->res_buf_bytes);
    for (size_t i = 0; i < n; i++) b->res_off[i] = ranges[i].first;
    b->res_out = (uint8_t *)device_base;
    if (b->resized) {
        set_result_offsets(b, b->res_off);
    } else {
        PjdDevImage *h_images = reinterpret_cast<PjdDevImage *>(b->h_in + b->images_off);
        for (size_t i = 0; i < n; i++) P.images[i].out_off = h_images[i].out_off = ranges[i].first;
        b->dev.out = (uint8_t *)device_base;
    }
    b->bound = true;
    b->bound_offsets = offsets != nullptr;
    b->bound_capacity = capacity;
    return PJD_OK;
}

int pjd_resize_tap(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *i0, uint32_t *i1, uint32_t *w)
{
    if (src_n == 0 || src_n > 65535u || dst_n == 0 || dst_n > 65535u || i >= dst_n) return PJD_E_ARG;
    uint32_t a, c, d;
    pjd_resize_tap_calc(src_n, dst_n, i, a, c, d);
    if (i0) *i0 = a;
    if (i1) *i1 = c;
    if (w) *w = d;
    return PJD_OK;
}

// ---- PJD_F_LIBJPEG: the arithmetic on its own, host only (the inlines the kernels of pjd_k_backend_std.hip run) -----------------------
int pjd_libjpeg_idct(const int16_t coef[64], const uint16_t q[64], uint8_t out[64])
{
    if (!coef || !q || !out) return PJD_E_ARG;
    uint32_t ws[64];
    for (int c = 0; c < 8; c++) {
        uint32_t x[8], o[8];
        for (int j = 0; j < 8; j++) x[j] = pjd_lj_dequant(coef[j * 8 + c], q[j * 8 + c]);
        pjd_lj_idct1d(x, o);
        for (int j = 0; j < 8; j++) ws[j * 8 + c] = pjd_lj_descale<PJD_LJ_PASS1_SHIFT>(o[j]);
    }
    for (int r = 0; r < 8; r++) {
        uint32_t o[8];
        pjd_lj_idct1d(ws + r * 8, o);
        for (int j = 0; j < 8; j++) out[r * 8 + j] = (uint8_t)pjd_lj_sample(o[j]);
    }
    return PJD_OK;
}

// ... and the reduced transforms of PJD_F_LIBJPEG_SCALE_*: n x n samples of one unit, n = 8 (the function above), 4, 2 or 1
int pjd_libjpeg_idct_scaled(const int16_t coef[64], const uint16_t q[64], uint32_t n, uint8_t *out)
{
    if (!coef || !q || !out) return PJD_E_ARG;
    switch (n) {
        case 8: return pjd_libjpeg_idct(coef, q, out);
        case 4: pjd_lj_idct_unit<4>(coef, q, out); return PJD_OK;
        case 2: pjd_lj_idct_unit<2>(coef, q, out); return PJD_OK;
        case 1: out[0] = (uint8_t)pjd_lj_sample_1x1(pjd_lj_dequant(coef[0], q[0])); return PJD_OK;
        default: return PJD_E_ARG;
    }
}

int pjd_libjpeg_ycc_to_rgb(uint8_t y, uint8_t cb, uint8_t cr, uint8_t rgb[3])
{
    if (!rgb) return PJD_E_ARG;
    int r, g, b;
    pjd_lj_ycc_to_rgb(y, cb, cr, r, g, b);
    rgb[0] = (uint8_t)r; rgb[1] = (uint8_t)g; rgb[2] = (uint8_t)b;
    return PJD_OK;
}

int pjd_libjpeg_upsample_row(const uint8_t *cur, const uint8_t *nb, int v, uint32_t n, uint8_t *out)
{
    (void)v;                             // which neighbour `nb` is (0: the row above, 1: the row below) changes nothing in the arithmetic
    if (!cur || !out || n == 0 || n > (1u << 30)) return PJD_E_ARG;
    for (uint32_t X = 0; X < 2 * n; X += 4) {
        int c[4];
        pjd_lj_upsample4(cur, nb, n, X, c);
        for (uint32_t k = 0; k < 4 && X + k < 2 * n; k++) out[X + k] = (uint8_t)c[k];
    }
    return PJD_OK;
}

int pjd_batch_set_views(pjd_batch *b, const uint32_t *picture_of_view, uint32_t n_views)
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (int rc = check_order(b, ST_VIEWS)) return rc;
    if (!picture_of_view) { ctx->err = "set_views: null view array"; return PJD_E_ARG; }
    if (n_views == 0 || n_views > PJD_MAX_VIEWS) { ctx->err = "set_views: the number of views must be 1..PJD_MAX_VIEWS"; return PJD_E_ARG; }
    if (P.out_format == PJD_OUT_BMP) { ctx->err = "set_views: a BMP batch takes no views (it takes no resample: PJD_OUT_RGB8, PJD_OUT_RGB8_PLANAR or PJD_OUT_GRAY8)"; return PJD_E_ARG; }
    const size_t n_pic = P.images.size();
    for (uint32_t v = 0; v < n_views; v++)
        if (picture_of_view[v] >= n_pic) {
            char buf[120];
            std::snprintf(buf, sizeof buf, "set_views: view %u names picture %u, the batch has %zu", v, picture_of_view[v], n_pic);
            ctx->err = buf;
            return PJD_E_ARG;
        }
    // from here on nothing fails.  Until the resample is set -- nothing can be bound, uploaded or decoded before -- an output's offset
    // and size are those of its picture in the batch's own buffer.
    b->view_pic.assign(picture_of_view, picture_of_view + n_views);
    b->viewed = true;
    std::vector<uint64_t> off(n_views), bytes(n_views);
    uint64_t sum = 0;
    for (uint32_t v = 0; v < n_views; v++) { off[v] = b->res_off[b->view_pic[v]]; bytes[v] = b->res_bytes[b->view_pic[v]]; sum += bytes[v]; }
    b->res_off = std::move(off); b->res_bytes = std::move(bytes);
    b->res_out_bytes = sum;
    return PJD_OK;
}

uint32_t pjd_batch_n_outputs(pjd_batch *b) { return b ? (uint32_t)b->n_out() : 0u; }

int pjd_batch_set_resize(pjd_batch *b, const uint32_t *out_w, const uint32_t *out_h)
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (int rc = check_order(b, ST_RESIZE)) return rc;
    if (!out_w || !out_h) { ctx->err = "set_resize: null size array"; return PJD_E_ARG; }
    if (P.out_format == PJD_OUT_BMP) { ctx->err = "set_resize: a BMP batch cannot be resized (PJD_OUT_RGB8 or PJD_OUT_RGB8_PLANAR)"; return PJD_E_ARG; }
    const size_t n = b->n_out();
    // the request: every output -- picture i, or view i of its picture -- from where the back end wrote its source at its decode size to
    // the packed layout of the result buffer (256-byte aligned offsets, as the planner lays out a batch's own buffer;
    // pjd_batch_bind_output may still change them)
    const uint32_t channels = b->back.gray() ? 1u : 3u;    // a grey batch is a planar batch with one plane
    const PjdPackedLayout lay = pjd_packed_layout(out_w, out_h, n, 1, channels);
    PjdResizeSpec spec;
    spec.planar = b->back.planes();
    spec.channels = channels;
    spec.out_w.assign(out_w, out_w + n); spec.out_h.assign(out_h, out_h + n);
    if (b->viewed) spec.view_pic = b->view_pic;
    size_t shard = n;                                      // the first output that reads a shard
    for (size_t i = 0; i < n; i++) {
        const uint32_t p = b->pic_of(i);
        const PjdDevImage &g = P.images[p];
        uint32_t sw = 0, sh = 0;
        pjd_scaled_dims(g.width, g.height, PJD_IF_OUT_SCALE_LOG(g.flags) << 4, &sw, &sh);
        spec.pic.push_back(PjdResizePicture{g.out_off, lay.off[i], sw, sh, g.out_stride});
        if (P.host[p].shard && shard == n) shard = i;
    }
    PjdResizeWork w;
    const PjdResizeFault f = pjd_resize_resolve(spec, w);
    // picture by picture: its size, then whether it is a shard; the batch as a whole behind them
    if (shard < n && !(f.picture >= 0 && (size_t)f.picture <= shard)) { ctx->err = fmt_name("set_resize: %s is a shard (its picture is only partly written)", b->out_name(shard)); return PJD_E_ARG; }
    if (!f.text.empty()) { ctx->err = "set_resize: " + f.text; return PJD_E_ARG; }
    hipSetDevice(ctx->device);
    void *d_res = nullptr;                                 // the result buffer first: the batch is as it was until everything is taken
    int rc = pool_dev_alloc(ctx, &d_res, (size_t)lay.buf_bytes, b->dev_blocks);
    if (rc == PJD_OK) rc = commit_request(b, spec, w);
    if (rc != PJD_OK) return rc;                           // what was taken stays with the batch until it is destroyed
    b->device_bytes += lay.buf_bytes;
    b->res_out = (uint8_t *)d_res;
    b->res_off = lay.off; b->res_bytes = lay.bytes;
    b->res_buf_bytes = lay.buf_bytes; b->res_out_bytes = lay.sum;
    b->resized = true;
    return PJD_OK;
}

int pjd_resize_aa_taps(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *first, uint32_t *count, uint32_t *q)
{
    if (src_n == 0 || src_n > 65535u || dst_n == 0 || dst_n > 65535u || i >= dst_n || src_n > 16u * dst_n) return PJD_E_ARG;
    uint32_t f, w[PJD_AA_MAX_TAPS];
    const uint32_t n = pjd_resize_aa_taps_calc(src_n, dst_n, i, f, w);
    if (first) *first = f;
    if (count) *count = n;
    if (q) std::memcpy(q, w, n * sizeof(uint32_t));
    return PJD_OK;
}

int pjd_resize_bicubic_taps(uint32_t src_n, uint32_t dst_n, uint32_t i, uint32_t *first, uint32_t *count, int32_t *q)
{
    if (src_n == 0 || src_n > 65535u || dst_n == 0 || dst_n > 65535u || i >= dst_n || src_n > 16u * dst_n) return PJD_E_ARG;
    uint32_t f;
    int32_t w[PJD_BICUBIC_MAX_TAPS];
    const uint32_t n = pjd_resize_bicubic_taps_calc(src_n, dst_n, i, f, w);
    if (first) *first = f;
    if (count) *count = n;
    if (q) std::memcpy(q, w, n * sizeof(int32_t));
    return PJD_OK;
}

int pjd_batch_set_resize_filter(pjd_batch *b, int filter)
{
    if (!b) return PJD_E_ARG;
    if (int rc = check_order(b, ST_FILTER)) return rc;
    PjdResizeSpec spec = b->spec;
    spec.filter_set = true; spec.filter = filter;
    return apply_request(b, spec, "set_resize_filter");
}

namespace {

bool finite_f32(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    return (x & 0x7f800000u) != 0x7f800000u;
}

}  // namespace

int pjd_resize_window_check(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const pjd_resize_window *win, int filter)
{
    return pjd_resize_window_fault(sw, sh, tw, th, win, filter) ? PJD_E_ARG : PJD_OK;
}

int pjd_batch_set_orientation(pjd_batch *b, const uint8_t *orientation)
{
    if (!b) return PJD_E_ARG;
    if (int rc = check_order(b, ST_ORIENTATION)) return rc;
    if (!orientation) { b->ctx->err ="set_orientation: null orientation array"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.ori_set = true; spec.orientation.assign(orientation, orientation + spec.pic.size());
    return apply_request(b, spec, "set_orientation");
}

int pjd_batch_set_resize_window(pjd_batch *b, const pjd_resize_window *win)
{
    if (!b) return PJD_E_ARG;
    if (int rc = check_order(b, ST_WINDOW)) return rc;
    if (!win) { b->ctx->err ="set_resize_window: null record array"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.win_set = true; spec.win.assign(win, win + spec.pic.size());
    return apply_request(b, spec, "set_resize_window");
}

int pjd_warp_tap(const double m[6], uint32_t i, uint32_t j, int64_t *x0, int64_t *y0, uint32_t *wx, uint32_t *wy)
{
    PjdDevWarp rec;
    if (!m || i >= 65535u || j >= 65535u || pjd_warp_quantise(m, rec)) return PJD_E_ARG;
    int32_t a, c;
    uint32_t u, v;
    pjd_warp_tap_calc(rec, i, j, a, c, u, v);
    if (x0) *x0 = a;
    if (y0) *y0 = c;
    if (wx) *wx = u;
    if (wy) *wy = v;
    return PJD_OK;
}

int pjd_resize_affine_check(uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, const double m[6])
{
    return pjd_resize_affine_fault(sw, sh, tw, th, m) ? PJD_E_ARG : PJD_OK;
}

int pjd_batch_set_resize_affine(pjd_batch *b, const double (*m)[6], const uint8_t fill[3])
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    if (int rc = check_order(b, ST_AFFINE)) return rc;
    // what the batch took before decides first: the rule, and its text, are the resolver's
    if (const char *other = pjd_resize_affine_excludes(b->spec)) return refuse(b, std::string("set_resize_affine after ") + other + ": the two exclude each other on one batch (multiply it into the matrix)");
    if (!m) { ctx->err = "set_resize_affine: null matrix array"; return PJD_E_ARG; }
    if (!fill) { ctx->err = "set_resize_affine: null fill"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.affine_set = true;
    spec.affine.resize(spec.pic.size());
    for (size_t i = 0; i < spec.pic.size(); i++) std::memcpy(spec.affine[i].m, m[i], sizeof spec.affine[i].m);
    std::memcpy(spec.affine_fill, fill, 3);
    return apply_request(b, spec, "set_resize_affine");
}

int pjd_colour_check(const double m[12])
{
    PjdDevColour rec;
    return m && !pjd_colour_quantise(m, rec) ? 1 : 0;
}

int pjd_colour_value(const double m[12], const uint8_t rgb[3], uint8_t out[3])
{
    PjdDevColour rec;
    if (!m || !rgb || !out || pjd_colour_quantise(m, rec)) return PJD_E_ARG;
    for (int c = 0; c < 3; c++) out[c] = (uint8_t)pjd_colour_calc(rec.q[c], rec.o[c] + 32768, rgb[0], rgb[1], rgb[2]);
    return PJD_OK;
}

int pjd_batch_set_colour(pjd_batch *b, const double (*m)[12])
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    if (int rc = check_order(b, ST_COLOUR)) return rc;
    if (b->back.gray()) { ctx->err = "set_colour: a grey batch has no colour map (one plane: gain and offset are pjd_batch_set_normalize's)"; return PJD_E_ARG; }
    if (!m) { ctx->err = "set_colour: null matrix array"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.colour_set = true;
    spec.colour.resize(spec.pic.size());
    for (size_t i = 0; i < spec.pic.size(); i++) std::memcpy(spec.colour[i].m, m[i], sizeof spec.colour[i].m);
    return apply_request(b, spec, "set_colour");
}

int pjd_blur_check(const pjd_blur *blur) { return pjd_blur_fault(blur) ? 0 : 1; }

int pjd_blur_taps(uint32_t ksize, double sigma, uint32_t *q)
{
    const pjd_blur e{sigma, ksize, 0u};
    if (!q || ksize == 0 || pjd_blur_fault(&e)) return PJD_E_ARG;
    pjd_blur_taps_calc(ksize, sigma, q);
    return PJD_OK;
}

int pjd_blur_index(uint32_t n, int64_t i, uint32_t *src)
{
    if (!src || n == 0 || n > 65535u) return PJD_E_ARG;
    const int64_t p = n > 1u ? 2 * ((int64_t)n - 1) : 1;  // the period: the rule folds by it, so does the 64-bit index before it is narrowed
    *src = pjd_blur_index_calc(n, (int32_t)(i % p));
    return PJD_OK;
}

int pjd_batch_set_blur(pjd_batch *b, const pjd_blur *blur)
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    if (int rc = check_order(b, ST_BLUR)) return rc;
    if (!blur) { ctx->err = "set_blur: null record array"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.blur_set = true;
    spec.blur.assign(blur, blur + spec.pic.size());
    return apply_request(b, spec, "set_blur");
}

int pjd_resize_pad_check(uint32_t out_w, uint32_t out_h, const pjd_resize_pad *pad)
{
    return pjd_resize_pad_fault(out_w, out_h, pad) ? PJD_E_ARG : PJD_OK;
}

int pjd_batch_set_resize_pad(pjd_batch *b, const pjd_resize_pad *pad, const uint8_t fill[3])
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    if (int rc = check_order(b, ST_PAD)) return rc;
    if (!pad) { ctx->err = "set_resize_pad: null record array"; return PJD_E_ARG; }
    if (!fill) { ctx->err = "set_resize_pad: null fill"; return PJD_E_ARG; }
    PjdResizeSpec spec = b->spec;
    spec.pad_set = true; spec.pad.assign(pad, pad + spec.pic.size());
    const int rc = apply_request(b, spec, "set_resize_pad");
    if (rc == PJD_OK) std::memcpy(b->pad_fill, fill, 3);
    return rc;
}

int pjd_batch_set_pad_value(pjd_batch *b, const float value[3])
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    if (int rc = check_order(b, ST_PAD_VALUE)) return rc;
    if (!value) { ctx->err = "set_pad_value: null value array"; return PJD_E_ARG; }
    for (int c = 0; c < 3; c++)
        if (!finite_f32(value[c])) { ctx->err = "set_pad_value: the values must be finite"; return PJD_E_ARG; }
    for (int c = 0; c < 3; c++) b->pad_value[c] = value[c];
    b->pad_value_set = true;
    return PJD_OK;
}

int pjd_normalize_value(int dtype, uint32_t v, float scale, float bias, void *out)
{
    if (dtype != PJD_DT_F16 && dtype != PJD_DT_BF16 && dtype != PJD_DT_F32) return PJD_E_ARG;
    if (v > 255u || !finite_f32(scale) || !finite_f32(bias) || !out) return PJD_E_ARG;
    const uint32_t e = pjd_f32_to_dtype_bits(dtype, pjd_normalize_f32(v, scale, bias));
    if (dtype == PJD_DT_F32) { std::memcpy(out, &e, 4); return PJD_OK; }
    const uint16_t h = (uint16_t)e;
    std::memcpy(out, &h, 2);
    return PJD_OK;
}

int pjd_batch_set_normalize(pjd_batch *b, int dtype, const float scale[3], const float bias[3])
{
    if (!b) return PJD_E_ARG;
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    if (int rc = check_order(b, ST_NORMALIZE)) return rc;
    if (!scale || !bias) { ctx->err = "set_normalize: null constant array"; return PJD_E_ARG; }
    if (dtype != PJD_DT_F16 && dtype != PJD_DT_BF16 && dtype != PJD_DT_F32) { ctx->err = "set_normalize: unknown dtype (PJD_DT_F16, PJD_DT_BF16 or PJD_DT_F32)"; return PJD_E_ARG; }
    for (int c = 0; c < 3; c++)
        if (!finite_f32(scale[c]) || !finite_f32(bias[c])) { ctx->err = "set_normalize: scale and bias must be finite"; return PJD_E_ARG; }
    if (P.out_format == PJD_OUT_BMP) { ctx->err = "set_normalize: a BMP batch cannot be normalised (PJD_OUT_RGB8 or PJD_OUT_RGB8_PLANAR)"; return PJD_E_ARG; }
    const size_t n = b->n_out();
    for (size_t i = 0; i < n; i++)
        if (P.host[b->pic_of(i)].shard) { ctx->err = fmt_name("set_normalize: %s is a shard (its picture is only partly written)", b->out_name(i)); return PJD_E_ARG; }
    hipSetDevice(ctx->device);
    // the result buffer in elements of the new size: packed, 256-byte aligned offsets.  Taken before anything changes: a failure
    // leaves the batch as it was (but for a block that stays with it until it is destroyed).
    std::vector<uint32_t> w = b->spec.out_w, h = b->spec.out_h;
    if (!b->resized) {
        w.resize(n); h.resize(n);
        for (size_t i = 0; i < n; i++) {                      // every output at its own picture's output size
            const PjdDevImage &g = P.images[b->pic_of(i)];
            pjd_scaled_dims(g.width, g.height, PJD_IF_OUT_SCALE_LOG(g.flags) << 4, &w[i], &h[i]);
        }
    }
    const PjdPackedLayout lay = pjd_packed_layout(w.data(), h.data(), n, PJD_DT_SIZE(dtype), P.gray ? 1u : 3u);
    void *d_res = nullptr;
    int rc = pool_dev_alloc(ctx, &d_res, (size_t)lay.buf_bytes, b->dev_blocks);
    if (rc != PJD_OK) return rc;
    b->device_bytes += lay.buf_bytes;
    if (!b->resized) {
        // no resize set: the identity resample (every tap weight 0) of every picture (every view: of its picture) at its own output size
        rc = pjd_batch_set_resize(b, w.data(), h.data());
        if (rc != PJD_OK) { give_back(b, d_res, lay.buf_bytes); return rc; }
    }
    give_back(b, b->res_out, b->res_buf_bytes);            // the uint8 result buffer of the resize
    set_result_offsets(b, lay.off);
    b->res_out = (uint8_t *)d_res;
    b->res_off = lay.off; b->res_bytes = lay.bytes;
    b->res_buf_bytes = lay.buf_bytes; b->res_out_bytes = lay.sum;
    b->norm.dtype = dtype;
    for (int c = 0; c < 3; c++) { b->norm.scale[c] = scale[c]; b->norm.bias[c] = bias[c]; }
    return PJD_OK;
}

void *pjd_host_alloc(uint64_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void pjd_host_free(void *p) { if (p) hipHostFree(p); }

// everything of a pjd_batch_info that the plan alone decides, the rest zero (pjd_plan_info, pjd_batch_get_info)
static void plan_info(const PjdPlan &P, pjd_batch_info *info)
{
    std::memset(info, 0, sizeof *info);
    info->n_images = (int32_t)P.images.size();
    info->pixels = P.pixels; info->ecs_bytes = P.ecs_bytes; info->out_bytes = P.out_bytes;
    info->coef_bytes = P.n_ent * 2 + P.n_words * 4 + P.dense_du * 128;      // lane streams + transposed words + dense scratch
    info->n_data_units = P.n_du;
    info->n_subsequences = P.subs.size();
    info->n_sequential = (int32_t)P.seq_images.size();
    info->sub_bytes = P.sub_bytes;
    info->plan_mode = (uint32_t)P.plan_mode;
    info->n_table_sets = (uint32_t)P.tsets.size();
    info->huff_lds_bytes = (uint32_t)(P.max_lut_bytes + PJD_HUFF_WAVES * (PJD_WAVE_LDS + PJD_PHASE_LDS) + 16);
    info->n_huff_waves = P.hwaves.size();
    info->n_huff_workgroups = P.hwgs.size();
    info->dc_plan = (P.dc_per_picture ? 1u : 0u) | ((uint32_t)P.groups.size() << 8);      // PJD_MAX_GROUPS fits the eight bits
}

// PJD_DEBUG_STATS: what the runtime makes of the entropy decoder's LDS, and the wave timeline of the last decode, to stderr
static void print_wave_timeline(const pjd_batch *b)
{
    int wg = 0;
    size_t lds = 0;
    if (pjd_huff_lanes_occupancy(b->dev, &wg, &lds) == hipSuccess)
        std::fprintf(stderr, "[pjd waves] pjd_k_huff_lanes: %zu B of LDS per workgroup, %d workgroups per CU\n", lds, wg);
    if (b->decoded) {                        // wave timeline of the last decode (units of 10 ns)
        const size_t nw = b->plan.hwaves.size();
        std::vector<uint32_t> d(nw * 32);
        if (hipMemcpy(d.data(), b->dev.dbg, d.size() * 4, hipMemcpyDeviceToHost) == hipSuccess && nw) {
            if (const char *dump = std::getenv("PJD_DEBUG_DUMP")) {          // the raw timeline (32 words per wave) for offline analysis
                if (FILE *f = std::fopen(dump, "wb")) { std::fwrite(d.data(), 4, d.size(), f); std::fclose(f); }
            }
            uint32_t t0 = d[0];
            for (size_t k = 0; k < nw; k++) if ((int32_t)(d[k * 32] - t0) < 0) t0 = d[k * 32];
            double sum[6] = {0}; uint32_t mx[6] = {0}; size_t worst = 0; uint32_t worst_end = 0;
            for (size_t k = 0; k < nw; k++) {
                const uint32_t *e = &d[k * 32];
                uint32_t end = e[0] - t0;
                for (int q = 1; q <= 5; q++) { sum[q] += e[q]; if (e[q] > mx[q]) mx[q] = e[q]; end += e[q]; }
                sum[0] += e[0] - t0; if (e[0] - t0 > mx[0]) mx[0] = e[0] - t0;
                if (end > worst_end) { worst_end = end; worst = k; }
            }
            const double n = (double)nw;
            {   // shader clock held during the kernel: cycles per 10 ns of every wave (bits 8.. of word 7), median
                std::vector<uint32_t> cl;
                for (size_t k = 0; k < nw; k++) { cl.push_back(d[k * 32 + 7] >> 8); d[k * 32 + 7] &= 0xffu; }
                std::sort(cl.begin(), cl.end());
                std::fprintf(stderr, "[pjd waves] shader clock while the waves ran: median %.2f GHz (min %.2f, max %.2f)\n", cl[nw / 2] / 160.0, cl.front() / 160.0, cl.back() / 160.0);
            }
            std::fprintf(stderr, "[pjd waves] n %zu | mean(us): start %.1f passA %.1f rounds %.1f stitch %.1f scan %.1f write+verify %.1f | max(us): %.1f %.1f %.1f %.1f %.1f %.1f\n",
                         nw, sum[0] / n / 100, sum[1] / n / 100, sum[2] / n / 100, sum[3] / n / 100, sum[4] / n / 100, sum[5] / n / 100,
                         mx[0] / 100.0, mx[1] / 100.0, mx[2] / 100.0, mx[3] / 100.0, mx[4] / 100.0, mx[5] / 100.0);
            const uint32_t *e = &d[worst * 32];
            std::fprintf(stderr, "[pjd waves] last to finish: wave %zu (image %u, %u lanes) start %.1f passA %.1f rounds %.1f stitch %.1f scan %.1f write %.1f -> end %.1f us\n",
                         worst, e[6], e[7], (e[0] - t0) / 100.0, e[1] / 100.0, e[2] / 100.0, e[3] / 100.0, e[4] / 100.0, e[5] / 100.0, worst_end / 100.0);
            // the waves of that image
            for (size_t k = 0; k < nw; k++)
                if (d[k * 32 + 6] == e[6] && d[k * 32 + 7] != 0) {
                    std::fprintf(stderr, "[pjd waves]   wave %zu: start %.1f passA %.1f rounds %.1f stitch %.1f scan %.1f write %.1f\n", k,
                                 (d[k * 32] - t0) / 100.0, d[k * 32 + 1] / 100.0, d[k * 32 + 2] / 100.0, d[k * 32 + 3] / 100.0, d[k * 32 + 4] / 100.0, d[k * 32 + 5] / 100.0);
                    std::fprintf(stderr, "[pjd waves]     rounds (lanes:us):");
                    for (int r = 0; r < 24 && d[k * 32 + 8 + r]; r++) {        // a walk (pjd_k_huffman.hip, walk_lane) is printed as w<lanes walked>
                        const uint32_t v = d[k * 32 + 8 + r];
                        std::fprintf(stderr, (v >> 31) ? " w%u:%.1f" : " %u:%.1f", (v >> 24) & 0x7fu, (v & 0xffffff) / 100.0);
                    }
                    std::fprintf(stderr, "\n");
                }
        }
    }
}

int pjd_batch_get_info(pjd_batch *b, pjd_batch_info *info)
{
    if (!b || !info) return PJD_E_ARG;
    hipSetDevice(b->ctx->device);
    plan_info(b->plan, info);
    info->out_bytes = b->res_out_bytes;                       // the results: resized, normalised or views where the batch has them
    info->device_bytes = b->device_bytes;
    info->n_fallback = b->n_fallback; info->exact_fallback_ms = b->exact_fallback_ms; info->n_entropy_errors = b->n_entropy_errors;
    // on the batch's own stream into page-locked memory: a plain hipMemcpy would wait for every other stream of the
    // device (it made the slots of the pipelined batcher run in lockstep, profiles/r02_pcie.md)
    unsigned long long *st = b->h_stats;
    if (b->decoded && hipMemcpyAsync(st, b->dev.stats, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->ctx->stream) == hipSuccess &&
        hipStreamSynchronize(b->ctx->stream) == hipSuccess) {
        info->sync_rounds = st[0]; info->sync_lane_passes = st[1]; info->fix_rounds = st[2]; info->fix_lane_passes = st[3];
        info->walks = st[PJD_STAT_WALKS]; info->walk_lanes = st[PJD_STAT_WALKS + 1];
        for (int r = 0; r < PJD_FLAG_REASONS && r < 8; r++) info->flag_waves[r] = st[PJD_STAT_FLAG0 + r];
        info->n_entries = st[PJD_STAT_ENTRIES];               // entries the lanes emitted in the last decode
        info->n_steps = st[PJD_STAT_STEPS];                   // ... in this many steps of the write pass
        info->lane_fill_x1024 = (uint32_t)st[PJD_STAT_FILL];  // the fullest lane region
    }
    if (b->dev.dbg) print_wave_timeline(b);
    return PJD_OK;
}

int pjd_plan_info(const pjd_image_desc *images, int n_images, int out_format, pjd_batch_info *info)
{
    if (!info) return PJD_E_ARG;
    PjdPlan P;
    std::string err;
    int rc = pjd_make_plan(images, n_images, out_format, P, err, env_sub_bytes(), env_plan_mode());      // as a context opened now would plan
    if (rc != PJD_OK) return rc;
    plan_info(P, info);
    return PJD_OK;
}

int pjd_plan_check(const pjd_image_desc *images, int n_images, int out_format, char *text, uint64_t cap)
{
    PjdPlan P;
    std::string err;
    const int rc = pjd_make_plan(images, n_images, out_format, P, err);
    if (text && cap) std::snprintf(text, (size_t)cap, "%s", rc == PJD_OK ? "" : err.c_str());
    return rc;
}

int pjd_plan_step_bits(const pjd_image_desc *image, uint32_t *step_bits_x256)
{
    if (!image || !step_bits_x256) return PJD_E_ARG;
    PjdPlan P;
    std::string err;
    int rc = pjd_make_plan(image, 1, PJD_OUT_RGB8, P, err);
    if (rc != PJD_OK) return rc;
    if (P.images.empty() || P.tset_step_bits.empty() || (P.images[0].flags & PJD_IF_SEQUENTIAL)) return PJD_E_ARG;   // no lane streams for this picture
    *step_bits_x256 = P.tset_step_bits[P.images[0].tset];
    return PJD_OK;
}

int pjd_plan_luts(const pjd_image_desc *image, void *blob, uint64_t cap, uint32_t *real_bytes, uint32_t *nominal_bytes, uint8_t *slots)
{
    if (!image || !real_bytes || !nominal_bytes) return PJD_E_ARG;
    PjdPlan P;
    std::string err;
    int rc = pjd_make_plan(image, 1, PJD_OUT_RGB8, P, err);
    if (rc != PJD_OK) return rc;
    if (P.images.empty() || P.tsets.empty() || (P.images[0].flags & PJD_IF_PROGRESSIVE)) return PJD_E_ARG;   // no table set: the scans bring their tables
    const PjdDevImage &im = P.images[0];
    const PjdDevTset &T = P.tsets[im.tset];
    *real_bytes = T.lut_bytes;
    *nominal_bytes = P.tset_nominal_bytes[im.tset];
    if (slots) std::memcpy(slots, im.tbl_slot, 6);
    if (!blob || T.lut_bytes == 0) return PJD_OK;
    if (cap < T.lut_bytes) return PJD_E_ARG;
    std::memset(blob, 0, T.lut_bytes);
    uint16_t *b16 = static_cast<uint16_t *>(blob);
    for (uint32_t slot = 0; slot < T.n_tables; slot++) {              // as one block of pjd_k_build_tables
        const PjdDevHuffRaw &r = P.tables[(size_t)im.tset * PJD_MAX_TABLES + slot];
        const uint32_t partner = r.is_ac ? slot : (uint32_t)T.pair_ac[slot];
        const bool has_partner = partner < T.n_tables;
        const PjdDevHuffRaw &r2 = P.tables[(size_t)im.tset * PJD_MAX_TABLES + (has_partner ? partner : slot)];
        uint32_t first[17], first2[17];
        pjd_lut_first_codes(r, first);
        pjd_lut_first_codes(r2, first2);
        uint32_t *L1 = reinterpret_cast<uint32_t *>(b16 + slot * (PJD_L1_BYTES / 2));
        const uint16_t *cp = T.l2_cp[slot], *ce = T.l2_ce[slot];
        const uint32_t p1 = T.l2_p1[slot];
        for (uint32_t idx = 0; idx < (1u << PJD_LUT_BITS); idx++)
            L1[idx] = pjd_lut_l1_entry(r, first, has_partner ? &r2 : nullptr, first2, cp, ce, p1, idx);
        const uint32_t n2 = pjd_lut_l2_entries(cp, p1);
        for (uint32_t j = 0; j < n2; j++) b16[ce[0] + j] = (uint16_t)pjd_lut_l2_entry(r, first, cp, ce, j);
    }
    return PJD_OK;
}

int pjd_batch_huff_occupancy(pjd_batch *b, int32_t *workgroups_per_cu, uint32_t *lds_bytes)
{
    if (!b || !workgroups_per_cu) return PJD_E_ARG;
    hipSetDevice(b->ctx->device);
    int n = 0;
    size_t lds = 0;
    if (pjd_huff_lanes_occupancy(b->dev, &n, &lds) != hipSuccess) return PJD_E_HIP;
    *workgroups_per_cu = n;
    if (lds_bytes) *lds_bytes = (uint32_t)lds;
    return PJD_OK;
}

uint64_t pjd_batch_output_size(pjd_batch *b, int image)
{
    if (!b || image < 0 || (size_t)image >= b->n_out()) return 0;
    return b->res_bytes[image];
}

void *pjd_batch_device_output(pjd_batch *b, int image)
{
    if (!b || image < 0 || (size_t)image >= b->n_out()) return nullptr;
    return b->res_out + b->res_off[image];
}

void *pjd_batch_device_status(pjd_batch *b) { return b ? (void *)b->dev.status : nullptr; }

uint64_t pjd_coefficients_size(uint32_t width, uint32_t height, uint8_t h_samp, uint8_t v_samp)
{
    // reference src/jpeg_scanner.cpp:257-262 (mcu_*_real) and src/decoder_host.cpp:125-128 (DPUs needed, 100 positions each)
    uint64_t w = (width + 7) / 8, h = (height + 7) / 8;
    if (h_samp == 2 && (w & 1)) w++;
    if (v_samp == 2 && (h & 1)) h++;
    const uint64_t pw = (w + 1) / 2 * 2, ph = (h + 1) / 2 * 2;
    return (pw * ph + 99) / 100 * 19200;
}

int pjd_batch_download_coefficients(pjd_batch *b, int image, int16_t *out, uint64_t capacity_int16)
{
    if (!b || !out || image < 0 || (size_t)image >= b->plan.images.size()) return PJD_E_ARG;
    if (!b->decoded) { b->ctx->err = "download_coefficients before decode"; return PJD_E_STATE; }
    pjd_ctx *ctx = b->ctx;
    PjdPlan &P = b->plan;
    hipSetDevice(ctx->device);
    int rc = settle(b);
    if (rc != PJD_OK) return rc;
    const PjdDevImage &g = P.images[image];
    const uint64_t n16 = pjd_coefficients_size(g.width, g.height, (uint8_t)g.hs, (uint8_t)g.vs);
    if (capacity_int16 < n16) { ctx->err = "download_coefficients: buffer smaller than pjd_coefficients_size"; return PJD_E_ARG; }
    hipStream_t s = ctx->stream;
    Scratch tmp;
    int16_t *d_out = nullptr;
    if (tmp.alloc(d_out, n16 * sizeof(int16_t)) != hipSuccess) { ctx->err = "hipMalloc failed (coefficients)"; return PJD_E_NOMEM; }
    hipError_t e = poison_dev(ctx, d_out, n16 * sizeof(int16_t));
    pjd_launch_zero(s, d_out, n16 * sizeof(int16_t));                  // 19200 int16 per DPU: a multiple of 16 bytes
    const uint32_t n_du = (g.last_mcu - g.first_mcu) * g.dus_per_mcu, first_du = g.first_mcu * g.dus_per_mcu;
    const bool routed = P.host[image].sequential;
    const bool fell_back = !routed && (b->h_status[image] & PJD_STW_NEEDS_EXACT);
    const uint32_t one = (uint32_t)image; const uint64_t zero = 0;     // the fallback's list and base: read until the stream is drained below
    if (routed) {
        pjd_launch_coefdump_dense(s, b->dev, (uint32_t)image, b->dev.coef + g.dense_base * 64, first_du, n_du, d_out);
    } else if (fell_back) {
        // the scratch settle() used is gone: run the exact kernel for this one image again (its status word does not change)
        PjdDevBatch dv;
        uint8_t *d[4];
        if (e == hipSuccess) e = redo_exact(b, tmp, &one, &zero, 1, n_du, nullptr, 0, nullptr, dv, d);
        if (tmp.out_of_memory) { ctx->err = "hipMalloc failed (coefficients scratch)"; return PJD_E_NOMEM; }
        if (e == hipSuccess) pjd_launch_coefdump_dense(s, dv, (uint32_t)image, dv.coef, first_du, n_du, d_out);
    } else {
        pjd_launch_coefdump_lanes(s, b->dev, (uint32_t)image, g.n_iwg, d_out);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n16 * sizeof(int16_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { ctx->err = std::string("download_coefficients: ") + hipGetErrorString(e); return PJD_E_HIP; }
    return PJD_OK;
}

// for pjd_split.hip, whose per-rank buffers are allocations on behalf of a context too: PJD_DEBUG_POISON's fill (no part of the ABI)
int pjd_debug_poison_fill(pjd_ctx *ctx, void *p, uint64_t bytes)
{
    if (!ctx) return PJD_E_ARG;
    return poison_dev(ctx, p, (size_t)bytes) == hipSuccess ? PJD_OK : PJD_E_HIP;
}

int pjd_decode_batch(pjd_ctx *ctx, const pjd_image_desc *images, int n_images, int out_format,
                     uint8_t *const *out, int32_t *status)
{
    pjd_batch *b = nullptr;
    int rc = pjd_batch_create(ctx, images, n_images, out_format, &b);
    if (rc != PJD_OK) return rc;
    rc = pjd_batch_upload(b);
    if (rc == PJD_OK) rc = pjd_batch_decode(b);
    if (rc == PJD_OK) rc = pjd_batch_download(b, out, status);
    pjd_batch_destroy(b);
    return rc;
}

int pjd_exec_dpu_payload(pjd_ctx *ctx, const uint32_t *metadata, int16_t *mcus, int n_dpus)
{
    if (!ctx || !metadata || !mcus || n_dpus < 0) return PJD_E_ARG;
    if (n_dpus == 0) return PJD_OK;
    for (int d = 0; d < n_dpus; d++) {
        const uint32_t *m = metadata + (size_t)d * 276;
        const uint32_t V = m[5] & 255, H = m[6] & 255;
        if (m[19] != 100 || m[4] > 3 || (V != 1 && V != 2) || (H != 1 && H != 2)) { ctx->err = "DPU metadata outside the supported envelope"; return PJD_E_ARG; }
        for (uint32_t c = 0; c < m[4]; c++) if ((m[7 + c] & 255) > 3) { ctx->err = "DPU metadata: quantisation table id > 3"; return PJD_E_ARG; }
    }
    hipSetDevice(ctx->device);
    Scratch tmp;
    uint32_t *dm = nullptr; int16_t *dc = nullptr;
    const size_t mb = (size_t)n_dpus * 276 * 4, cb = (size_t)n_dpus * 19200 * 2;
    if (const hipError_t e = tmp.alloc(dm, mb)) { ctx->err = std::string("hipMalloc((void **)&dm, mb): ") + hipGetErrorString(e); return PJD_E_HIP; }
    if (tmp.alloc(dc, cb) != hipSuccess) { ctx->err = "hipMalloc(mcus)"; return PJD_E_NOMEM; }
    int rc = PJD_OK;
    auto chk = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == PJD_OK) { ctx->err = std::string(what) + ": " + hipGetErrorString(e); rc = PJD_E_HIP; } };
    chk(poison_dev(ctx, dm, mb), "poison(metadata_buffer)");
    chk(poison_dev(ctx, dc, cb), "poison(mcus)");
    chk(hipMemcpyAsync(dm, metadata, mb, hipMemcpyHostToDevice, ctx->stream), "copy(metadata_buffer)");
    chk(hipMemcpyAsync(dc, mcus, cb, hipMemcpyHostToDevice, ctx->stream), "copy(mcus)");
    if (rc == PJD_OK) { pjd_launch_dpu_payload(ctx->stream, dm, dc, n_dpus); chk(hipGetLastError(), "exec"); }
    chk(hipMemcpyAsync(mcus, dc, cb, hipMemcpyDeviceToHost, ctx->stream), "copy back");
    chk(hipStreamSynchronize(ctx->stream), "sync");
    return rc;
}

}  // extern "C"
