// Shared internals of libfaceid.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/faceid.h"

namespace fid {

void set_error(const char *fmt, ...);

#define FID_HIP(call)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            fid::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return FID_E_HIP;                                                            \
        }                                                                                \
    } while (0)

#define FID_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            fid::set_error(__VA_ARGS__);       \
            return FID_E_INVALID;              \
        }                                      \
    } while (0)

#define FID_TRY(expr)                \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != FID_OK) return rc_; \
    } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Division of a non-negative int (< 2^31) by a launch-time constant as multiply-high + shift: the kernels decode
// (item -> image, tile row, tile column, cout block) several times per step, and a runtime integer division costs
// ~40 instructions each.  q = x / d  ==  d == 1 ? x : umulhi(x, mul) >> shr.
struct FastDiv {
    unsigned mul, shr, d;
};
inline FastDiv fastdiv_make(int d) {
    FastDiv f{0u, 0u, (unsigned)d};
    if (d > 1) {
        unsigned lg = 0;
        while ((1ull << lg) < (unsigned long long)d) lg++;      // ceil(log2(d))
        const unsigned p = 31 + lg;
        f.mul = (unsigned)(((1ull << p) + (unsigned)d - 1) / (unsigned)d);
        f.shr = p - 32;
    }
    return f;
}
#ifdef __HIPCC__
// Workgroup ids are dealt round-robin over the 8 XCDs (each with its own L2): position of workgroup b in XCD-major order, so
// that workgroups which share an L2 get CONSECUTIVE work items (neighbouring tiles share halo pixels, the cout blocks of one
// tile share its whole patch).  A bijection on [0, g); speed only, never correctness.
__device__ __forceinline__ int xcd_major_id(int b, int g) {
    const int q = g >> 3, r = g & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

__device__ __forceinline__ int fastdiv(int x, const FastDiv &f) { return f.d == 1 ? x : (int)(__umulhi((unsigned)x, f.mul) >> f.shr); }
#endif
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace fid

struct fid_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    std::mutex mu;
    // growable scratch arenas (never shrink; no allocation on the steady-state path)
    void *scratch[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // 0 post-process, 1 split-K partials, 2 / 3 match, 4 the autotuner's cache-flush buffer
    size_t scratch_bytes[5] = {0, 0, 0, 0, 0};
    hipEvent_t events[FID_MAX_EVENTS] = {};
    hipStream_t copy_stream = nullptr;   // H2D uploads that overlap compute (video front-end)
    hipEvent_t copy_done = nullptr, compute_done = nullptr;
    hipEvent_t slot_uploaded[FID_UPLOAD_SLOTS] = {}, slot_released[FID_UPLOAD_SLOTS] = {};   // per staging buffer
    bool slot_has_upload[FID_UPLOAD_SLOTS] = {}, slot_has_release[FID_UPLOAD_SLOTS] = {};
    // SCRFD post-process state
    int cand_cap = 4096;
    int32_t *status_dev = nullptr;  // [0] max candidates seen, [1] max survivors seen
    int last_out_cap = 0;
    // per-image geometry table of the *_ragged entry points (fid::ragged_table): grows, never shrinks
    void *ragged_tab = nullptr;
    int ragged_tab_cap = 0;         // entries
    // tile table of the tiled detection entry points (fid::tile_table): grows, never shrinks
    void *tile_tab = nullptr;
    int tile_tab_cap = 0;           // entries
};

namespace fid {
// scratch arena `slot` with at least `bytes` bytes (grows by reallocating; contents undefined)
int get_scratch(fid_ctx *ctx, int slot, size_t bytes, void **out);
// give a scratch arena back (synchronises the stream first): the autotuner's 320 MB flush buffer does not outlive a tuning run
int release_scratch(fid_ctx *ctx, int slot);
// hipFuncAttributeMaxDynamicSharedMemorySize >= bytes for kernel `func` on the context's device.  The attribute is per device, so the
// largest value set so far is remembered per (kernel, device) -- under a mutex: contexts on several devices and several host
// threads launch the same kernels (a function-local static flag covered neither).
int ensure_dyn_lds(fid_ctx *ctx, const void *func, int bytes);

// One image of a mixed-size batch (the *_ragged entry points): where it lies in the caller's allocation and the letterbox geometry the
// host computed for it in double (reference models/scrfd.py:123-138).  Every stage reads the entry of its image by a block-uniform index.
struct RaggedImg {
    long long off;              // first byte of the image, relative to frames_dev
    int H, W;                   // the image
    int new_h, new_w;           // resized size inside the letterbox
    double scale_x, scale_y;    // W / new_w, H / new_h
    float det_scale;            // (float)(new_h / H): what the post-process divides by
    int mode;                   // letterbox: 0 bilinear, 1 identity copy, 2 exact 2x decimation (INTER_AREA)
};
static_assert(sizeof(RaggedImg) == 48, "RaggedImg is copied to the device as 48-byte entries");
// Letterbox geometry of one H x W image into in_h x in_w (scrfd.py:125-134 in double, int() truncation); false = degenerate.  The one
// statement of it: every letterbox, tile cut and post-process entry point takes its sizes, scales, det_scale and mode from here.  A
// degenerate image still gets its sizes and det_scale (fid_scrfd_postprocess refuses nothing and divides by it, as the reference does).
inline bool ragged_geometry(int H, int W, int in_h, int in_w, RaggedImg *g) {
    const double im_ratio = (double)H / (double)W, model_ratio = (double)in_h / (double)in_w;
    int new_h, new_w;
    if (im_ratio > model_ratio) { new_h = in_h; new_w = (int)((double)new_h / im_ratio); }
    else { new_w = in_w; new_h = (int)((double)new_w * im_ratio); }
    g->H = H; g->W = W; g->new_h = new_h; g->new_w = new_w;
    g->det_scale = (float)((double)new_h / (double)H);
    if (new_h <= 0 || new_w <= 0) return false;
    g->scale_x = (double)W / (double)new_w; g->scale_y = (double)H / (double)new_h;
    g->mode = (new_w == W && new_h == H) ? 1 : ((W == 2 * new_w && H == 2 * new_h) ? 2 : 0);
    return true;
}
// Copy B host entries into the context's device table, ordered on the context's stream: the entries travel as kernel arguments of
// small store kernels, so the host array is free when this returns, the write runs after every earlier reader of the table, and
// nothing synchronises with the host (the table only reallocates, behind a stream synchronise, when B outgrows it).
int ragged_table(fid_ctx *ctx, const RaggedImg *host, int B, const RaggedImg **dev);

// One tile of a tiled detection (fid_tile_cut / fid_scrfd_postprocess_tiled): a row of the caller's [T,6] table plus what the host derives
// from it.  kind 0 (native): the rectangle is copied 1:1, det_scale is exactly 1.0f.  kind 1 (letterboxed): the rectangle is resized with
// the geometry ragged_geometry computes for an h x w image.  Every stage reads the entry of its tile by a block-uniform index.
struct TileEntry {
    int frame, x0, y0, w, h, kind;
    int new_h, new_w;           // resized size inside the detector input (kind 0: h, w)
    double scale_x, scale_y;    // w / new_w, h / new_h
    float det_scale;            // what the post-process divides by
    int mode;                   // kind 1: RaggedImg::mode of the rectangle
    int rank;                   // position of the tile among its frame's tiles
    int pad_;
};
static_assert(sizeof(TileEntry) == 64, "TileEntry is copied to the device as 64-byte entries");
// Validate a host [T,6] table (frame, x0, y0, w, h, kind) against B frames of H x W and the detector input and fill the entries: all or
// nothing, FID_E_INVALID names the first bad row in fid_last_error().  max_per_frame: the largest number of tiles one frame has (may be NULL).
int tile_entries(const int32_t *tiles, int T, int B, int H, int W, int in_h, int in_w, std::vector<TileEntry> &tab, int *max_per_frame);
// ragged_table for tile entries: the same ordering and lifetime guarantees
int tile_table(fid_ctx *ctx, const TileEntry *host, int T, const TileEntry **dev);
}  // namespace fid
