// Tracking faces across the frames of a video, on the device: which detection continues which track, and which faces need an embedding now.
// Serves the reference's video loop (main.py:174-184, two cameras in main2.py:91-99), which embeds and matches every face of every frame:
// here a face that has been named keeps its name and is embedded again only every `refresh` frames.
//
// State (S streams x T <= 64 slots, include/faceid.h) lives in device memory in the layout fid_tracker_read returns.  Three kernels per step,
// ordered by the context's stream only -- no workgroup waits for another, nothing is polled, nothing is launched cooperatively:
//
//   track_walk      one wave64 per stream.  Lane l owns slot l for the whole walk, in registers: state is loaded once and stored once.  The
//                   wave visits the stream's frames in batch order; a frame's boxes are loaded 64 at a time (one per lane) and broadcast lane
//                   to lane.  Per detection: every lane scores its own track (the overlap arithmetic of postproc.hip's nms_select_frame,
//                   operation for operation), the wave takes the maximum of one 64-bit key (order-preserving bits of the overlap << 32 | ~slot:
//                   the best overlap at the lowest slot; 0 = no candidate -- visit_group.hip's idiom; a ballot spares the reduction when fewer
//                   than two tracks hit), and without a hit the lowest free slot comes from one ballot.  No barrier, no LDS, no atomics.  Writes track [B,cap,2] for the detections f < k_b and the number of
//                   EMBED-flagged faces per frame.
//   track_pack      one wave per frame: the frame's offset (every wave sums the per-frame counts before it: B / 64 loads per lane), then the
//                   flagged faces in rank order into the row table (ballot + popcount), in fid_face_pack's format; it also writes the {-1,-1}
//                   entries of track (f >= k_b, skipped frames) and the -1 rows behind the last row.
//   track_identify  (after fid_match) the walk's shape again: lane l owns slot l's identity; per frame the rows of the frame fold into their
//                   slots, then every detection reads its slot's identity with one indexed shuffle.
//
// This file must never get a fast-math flag: the overlap is specified with the correctly rounded divide (tests compare bit for bit).
#include <cmath>

#include "common.h"
#include "track_state.h"

namespace {

using fid::cdiv;

constexpr int SW = FID_TRACK_SLOT_WORDS;
constexpr int TAB_CHUNK = 960;               // int32 entries per store kernel: 3 840 of the 4 096 bytes a kernel's arguments may take
struct TabChunk { int32_t e[TAB_CHUNK]; };

__global__ void __launch_bounds__(256) track_tab_store(TabChunk c, int n, int32_t *dst) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.e[i];
}

// streams [s0, s0 + n): every slot free (id -1, every other word 0), next_id = lost = 0
__global__ void __launch_bounds__(256) track_reset(int32_t *slots, int32_t *streams, int s0, int n, int T) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < n * T * SW) slots[(size_t)s0 * T * SW + gid] = gid % SW == 0 ? -1 : 0;
    if (gid < n * 2) streams[s0 * 2 + gid] = 0;
}

__device__ __forceinline__ unsigned long long make_key(float ovr, int slot) {      // (only called for ovr > thresh >= 0: never NaN, never negative)
    return ((unsigned long long)(__float_as_uint(ovr) | 0x80000000u) << 32) | (unsigned)~(unsigned)slot;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long k, int m) {
    return ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), m) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, m);
}
// lane `l`'s value, l the same in every lane (a loop counter, a ballot's first bit): one v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(lane_i(__float_as_int(v), l)); }
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

struct WalkArgs {
    int32_t *slots, *streams;
    const int32_t *tab;                      // [B] stream of frame b
    int32_t *nemb;                           // [B] EMBED-flagged faces of frame b (written for the frames that are walked)
    const float *det;
    const int32_t *counts;
    int32_t *track;
    float thresh;
    int max_age, refresh, retry, B, cap, T;
};

__global__ void __launch_bounds__(64) track_walk(const WalkArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < a.T;
    int32_t *st = a.slots + ((size_t)s * a.T + (mine ? lane : 0)) * SW;
    int id = -1, missed = 0, since = 0;
    bool known = false;                      // named by the last identify; false for a track started during this call
    float bx1 = 0.f, by1 = 0.f, bx2 = 0.f, by2 = 0.f;
    if (mine) {
        id = st[0]; missed = st[1]; since = st[2]; known = st[3] >= 0;
        bx1 = __int_as_float(st[5]); by1 = __int_as_float(st[6]); bx2 = __int_as_float(st[7]); by2 = __int_as_float(st[8]);
    }
    int next_id = a.streams[s * 2], lost = a.streams[s * 2 + 1];      // (the same in every lane)
    for (int b = 0; b < a.B; b++) {
        if (a.tab[b] != s) continue;         // (wave-uniform)
        const int k = min(max(a.counts[b], 0), a.cap);
        bool matched = false;
        int n_embed = 0;
        for (int f0 = 0; f0 < k; f0 += 64) {
            const int n = min(64, k - f0);
            float dx1 = 0.f, dy1 = 0.f, dx2 = 0.f, dy2 = 0.f;
            if (lane < n) {
                const float *d = a.det + ((size_t)b * a.cap + f0 + lane) * 5;
                dx1 = d[0]; dy1 = d[1]; dx2 = d[2]; dy2 = d[3];
            }
            int out_id = -1, out_word = -1;
            for (int j = 0; j < n; j++) {
                const float x1 = lane_f(dx1, j), y1 = lane_f(dy1, j), x2 = lane_f(dx2, j), y2 = lane_f(dy2, j);
                unsigned long long key = 0ull;
                if (id >= 0 && !matched) {
                    const float area_t = __fmul_rn(__fadd_rn(__fsub_rn(bx2, bx1), 1.f), __fadd_rn(__fsub_rn(by2, by1), 1.f));
                    const float area_d = __fmul_rn(__fadd_rn(__fsub_rn(x2, x1), 1.f), __fadd_rn(__fsub_rn(y2, y1), 1.f));
                    const float xx1 = fmaxf(bx1, x1), yy1 = fmaxf(by1, y1), xx2 = fminf(bx2, x2), yy2 = fminf(by2, y2);
                    const float w_ = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f));
                    const float h_ = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
                    const float inter = __fmul_rn(w_, h_);
                    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_t, area_d), inter));
                    if (ovr > a.thresh) key = make_key(ovr, lane);           // strict: a NaN never hits
                }
                // the wave's maximum key = the best overlap at the lowest slot.  No hit and one hit -- nearly every detection of a video -- need
                // no reduction: the ballot says so, and the one hit's lane is the answer; the twelve dependent shuffles run only when several tracks hit
                const unsigned long long hits = __ballot(key != 0ull);
                if ((hits & (hits - 1ull)) != 0ull) {
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long t = shfl_xor_u64(key, o);
                        key = t > key ? t : key;
                    }
                }
                int tid, word;
                if (hits != 0ull) {          // (wave-uniform) the detection continues the track in `slot`
                    const int slot = (hits & (hits - 1ull)) != 0ull ? (int)~(unsigned)key : __ffsll((long long)hits) - 1;
                    int embed = 0;
                    if (lane == slot) {
                        bx1 = x1; by1 = y1; bx2 = x2; by2 = y2;
                        missed = 0; matched = true; since += 1;
                        if (since >= (known ? a.refresh : a.retry)) { embed = 1; since = 0; }
                    }
                    embed = lane_i(embed, slot);
                    tid = lane_i(id, slot);
                    word = slot | (embed ? FID_TRACK_EMBED : 0);
                    n_embed += embed;
                } else {
                    const unsigned long long free_mask = __ballot(mine && id == -1);
                    if (free_mask != 0ull) { // a new track in the lowest free slot
                        const int slot = __ffsll((long long)free_mask) - 1;
                        if (lane == slot) {
                            id = next_id; bx1 = x1; by1 = y1; bx2 = x2; by2 = y2;
                            missed = 0; since = 0; matched = true; known = false;
                        }
                        tid = next_id;
                        next_id += 1;
                        word = slot | FID_TRACK_STARTED | FID_TRACK_EMBED;
                    } else {                 // no slot left: untracked, embedded every frame
                        tid = -1; word = -1;
                        lost += 1;
                    }
                    n_embed += 1;
                }
                if (lane == j) { out_id = tid; out_word = word; }
            }
            if (lane < n) *(int2 *)(a.track + ((size_t)b * a.cap + f0 + lane) * 2) = make_int2(out_id, out_word);
        }
        if (id >= 0 && !matched) {           // end of frame
            missed += 1;
            if (missed > a.max_age) { id = -1; missed = 0; since = 0; known = false; bx1 = by1 = bx2 = by2 = 0.f; }
        }
        if (lane == 0) a.nemb[b] = n_embed;
    }
    if (mine) {                              // (words 3, 4 -- the identity -- belong to track_identify; word 9 stays 0)
        st[0] = id; st[1] = missed; st[2] = since;
        st[5] = __float_as_int(bx1); st[6] = __float_as_int(by1); st[7] = __float_as_int(bx2); st[8] = __float_as_int(by2);
    }
    if (lane == 0) { a.streams[s * 2] = next_id; a.streams[s * 2 + 1] = lost; }
}

// wave w < B: frame w; wave B: offsets[B].  All threads: the -1 rows behind the table's last row.
__global__ void __launch_bounds__(256) track_pack(const int32_t *__restrict__ tab, const int32_t *__restrict__ nemb,
                                                  const int32_t *__restrict__ counts, int32_t *__restrict__ track, int B, int cap,
                                                  int32_t *__restrict__ offsets, int32_t *__restrict__ src, int row_cap) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    int before = 0, total = 0;               // flagged faces of the frames before this wave's, and of all frames (<= B * cap: fits an int)
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        const int v = (b < B && tab[b] >= 0) ? nemb[b] : 0;
        total += v;
        before += b < w ? v : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { total += __shfl_xor(total, o); before += __shfl_xor(before, o); }
    if (w < B) {
        const int b = w;
        const int k = tab[b] >= 0 ? min(max(counts[b], 0), cap) : 0;
        if (lane == 0) offsets[b] = before;
        int pos = before;
        for (int f0 = 0; f0 < cap; f0 += 64) {
            const int f = f0 + lane;
            bool flag = false;
            if (f < k) flag = (track[((size_t)b * cap + f) * 2 + 1] & FID_TRACK_EMBED) != 0;      // (-1, an untracked face, carries the bit)
            else if (f < cap) *(int2 *)(track + ((size_t)b * cap + f) * 2) = make_int2(-1, -1);
            const unsigned long long m = __ballot(flag);
            const int r = pos + lanes_below(m, lane);
            if (flag && r < row_cap) src[r] = b * cap + f;
            pos += __popcll(m);
        }
    } else if (w == B && lane == 0) offsets[B] = total;
    const int nthreads = gridDim.x * 256;
    for (int i = min(total, row_cap) + blockIdx.x * 256 + (int)threadIdx.x; i < row_cap; i += nthreads) src[i] = -1;
}

struct IdentArgs {
    int32_t *slots;
    const int32_t *tab, *counts, *track, *offsets, *idx;
    const float *score;
    int32_t *out_idx;
    float *out_score;
    int n_rows, B, cap, S, T;                // n_rows: already min(n_rows, row_cap)
};

__global__ void __launch_bounds__(64) track_identify(const IdentArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < a.T;
    int32_t *st = a.slots + ((size_t)s * a.T + (mine ? lane : 0)) * SW;
    int ii = -1;
    float is = 0.f;
    if (mine) { ii = st[3]; is = __int_as_float(st[4]); }
    for (int b = 0; b < a.B; b++) {
        const int owner = a.tab[b];
        if (owner < 0) {                     // a skipped frame: (-1, 0) everywhere, written by wave b % S
            if (b % a.S == s)
                for (int f = lane; f < a.cap; f += 64) { a.out_idx[(size_t)b * a.cap + f] = -1; a.out_score[(size_t)b * a.cap + f] = 0.f; }
            continue;
        }
        if (owner != s) continue;            // (wave-uniform)
        const int k = min(max(a.counts[b], 0), a.cap);
        int pos = a.offsets[b];              // row of the frame's first flagged face; the i-th flagged face has row pos + i (= where src names it)
        for (int f0 = 0; f0 < a.cap; f0 += 64) {
            const int f = f0 + lane;
            const bool valid = f < k;
            int word = -1;
            if (valid) word = a.track[((size_t)b * a.cap + f) * 2 + 1];
            const bool flag = valid && (word & FID_TRACK_EMBED) != 0;
            const unsigned long long m = __ballot(flag);
            const int r = pos + lanes_below(m, lane);
            pos += __popcll(m);
            const bool has_row = flag && r < a.n_rows;
            const int ri = has_row ? a.idx[r] : -1;
            const float rs = has_row ? a.score[r] : 0.f;
            const bool tracked = valid && word >= 0;
            const int slot = word & 63;
            const bool started = tracked && (word & FID_TRACK_STARTED) != 0;
            // a slot occurs at most once per frame, so the order of the faces within the frame does not matter to their slots
            unsigned long long work = __ballot(tracked && (started || has_row));
            while (work != 0ull) {           // (wave-uniform)
                const int j = __ffsll((long long)work) - 1;
                work &= work - 1ull;
                const int sl = __shfl(slot, j), st_ = __shfl((int)started, j), hr = __shfl((int)has_row, j), ci = __shfl(ri, j);
                const float cs = __shfl(rs, j);
                if (lane == sl) {
                    if (st_) { ii = -1; is = 0.f; }
                    if (hr && ci >= 0 && cs > is) { ii = ci; is = cs; }
                }
            }
            const int ti = __shfl(ii, slot);
            const float ts = __shfl(is, slot);
            int oi = -1;
            float os = 0.f;
            if (tracked) { oi = ti; os = ts; }
            else if (has_row) { oi = ri; os = rs; }
            if (f < a.cap) { a.out_idx[(size_t)b * a.cap + f] = oi; a.out_score[(size_t)b * a.cap + f] = os; }
        }
    }
    if (mine) {                              // a slot that is free after the step keeps no identity
        const bool is_free = st[0] == -1;
        st[3] = is_free ? 0 : ii;
        st[4] = is_free ? 0 : __float_as_int(is);
    }
}

// the tracker's per-frame table holds at least B entries (twice: streams, flagged counts)
int tab_reserve(fid_ctx *ctx, fid_tracker *t, int B) {
    if (t->tab_cap >= B) return FID_OK;
    if (t->tab) {
        FID_HIP(hipStreamSynchronize(ctx->stream));
        FID_HIP(hipFree(t->tab));
        t->tab = nullptr;
        t->tab_cap = 0;
    }
    const int want = std::max(1024, B + B / 4);
    FID_HIP(hipMalloc((void **)&t->tab, (size_t)want * 2 * sizeof(int32_t)));
    t->tab_cap = want;
    return FID_OK;
}

int check_shape(const int32_t *stream, int B, int cap, int row_cap, int S) {
    FID_REQUIRE(B > 0 && cap > 0, "track: bad sizes B %d, cap %d", B, cap);
    FID_REQUIRE((long long)B * cap <= 0x7FFFFFFFll, "track: B * cap = %lld overflows the row table's int32 entries", (long long)B * cap);
    FID_REQUIRE(B <= 0x7FFFFFFF - 1024, "track: B %d too large", B);
    FID_REQUIRE(row_cap > 0, "track: row_cap %d must be positive", row_cap);
    for (int b = 0; b < B; b++) FID_REQUIRE(stream[b] < S, "track: stream[%d] = %d, the tracker has %d streams", b, stream[b], S);
    return FID_OK;
}

}  // namespace

extern "C" {

int fid_tracker_create(fid_ctx *ctx, int S, int T, fid_tracker **out) {
    FID_REQUIRE(ctx && out, "tracker: NULL argument");
    FID_REQUIRE(S >= 1 && (long long)S * FID_TRACK_MAX_SLOTS * SW <= 0x7FFFFFFFll, "tracker: %d streams", S);
    FID_REQUIRE(T >= 1 && T <= FID_TRACK_MAX_SLOTS, "tracker: %d slots per stream (1 .. %d)", T, FID_TRACK_MAX_SLOTS);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    fid_tracker *t = new fid_tracker();
    t->S = S; t->T = T; t->device = ctx->device;
    if (hipMalloc((void **)&t->slots, (size_t)S * T * SW * 4) != hipSuccess || hipMalloc((void **)&t->streams, (size_t)S * 2 * 4) != hipSuccess) {
        if (t->slots) (void)hipFree(t->slots);
        delete t;
        fid::set_error("tracker: out of device memory for %d x %d slots", S, T);
        return FID_E_NOMEM;
    }
    hipLaunchKernelGGL(track_reset, dim3(cdiv(S * T * SW, 256)), dim3(256), 0, ctx->stream, t->slots, t->streams, 0, S, T);
    FID_HIP(hipGetLastError());
    *out = t;
    return FID_OK;
}

int fid_tracker_destroy(fid_ctx *ctx, fid_tracker *trk) {
    FID_REQUIRE(ctx, "tracker: NULL context");
    if (!trk) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    if (trk->slots) (void)hipFree(trk->slots);
    if (trk->streams) (void)hipFree(trk->streams);
    if (trk->tab) (void)hipFree(trk->tab);
    delete trk;
    return FID_OK;
}

int fid_tracker_reset(fid_ctx *ctx, fid_tracker *trk, int stream) {
    FID_REQUIRE(ctx && trk, "tracker: NULL argument");
    FID_REQUIRE(stream >= -1 && stream < trk->S, "tracker: reset of stream %d, the tracker has %d", stream, trk->S);
    FID_REQUIRE(stream < 0 || !trk->pending, "tracker: reset of one stream between fid_track_step and its fid_track_identify");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    const int s0 = stream < 0 ? 0 : stream, n = stream < 0 ? trk->S : 1;
    hipLaunchKernelGGL(track_reset, dim3(cdiv(n * trk->T * SW, 256)), dim3(256), 0, ctx->stream, trk->slots, trk->streams, s0, n, trk->T);
    FID_HIP(hipGetLastError());
    if (stream < 0) trk->pending = false;    // (a pending step is dropped with the tracks it was about)
    return FID_OK;
}

int fid_tracker_read(fid_ctx *ctx, fid_tracker *trk, int32_t *slots_host, int32_t *streams_host) {
    FID_REQUIRE(ctx && trk && slots_host && streams_host, "tracker: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipMemcpyAsync(slots_host, trk->slots, (size_t)trk->S * trk->T * SW * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipMemcpyAsync(streams_host, trk->streams, (size_t)trk->S * 2 * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    return FID_OK;
}

int fid_track_step(fid_ctx *ctx, fid_tracker *trk, const float *det_dev, const int32_t *counts_dev, const int32_t *stream, int B, int cap,
                   const fid_track_config *cfg, int32_t *track_dev, int32_t *offsets_dev, int32_t *src_dev, int row_cap) {
    FID_REQUIRE(ctx && trk && det_dev && counts_dev && stream && cfg && track_dev && offsets_dev && src_dev, "track step: NULL argument");
    FID_TRY(check_shape(stream, B, cap, row_cap, trk->S));
    FID_REQUIRE(!std::isnan(cfg->iou_thresh) && cfg->iou_thresh >= 0.f && cfg->iou_thresh < 1.f, "track step: iou_thresh %g outside [0, 1)",
                (double)cfg->iou_thresh);
    FID_REQUIRE(cfg->max_age >= 0 && cfg->refresh >= 1 && cfg->retry >= 1, "track step: max_age %d must be >= 0, refresh %d and retry %d >= 1",
                cfg->max_age, cfg->refresh, cfg->retry);
    FID_REQUIRE(!trk->pending, "track step: the previous step's fid_track_identify has not been called");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_TRY(tab_reserve(ctx, trk, B));
    // the stream array travels as kernel arguments (like the per-image table of the mixed-size entry points): the caller's array is free
    // when this returns and nothing synchronises with the host
    TabChunk c;
    for (int b0 = 0; b0 < B; b0 += TAB_CHUNK) {
        const int n = std::min(TAB_CHUNK, B - b0);
        memcpy(c.e, stream + b0, (size_t)n * 4);
        if (n < TAB_CHUNK) memset(c.e + n, 0, (size_t)(TAB_CHUNK - n) * 4);
        hipLaunchKernelGGL(track_tab_store, dim3(1), dim3(256), 0, ctx->stream, c, n, trk->tab + b0);
    }
    WalkArgs a{};
    a.slots = trk->slots; a.streams = trk->streams; a.tab = trk->tab; a.nemb = trk->tab + trk->tab_cap;
    a.det = det_dev; a.counts = counts_dev; a.track = track_dev;
    a.thresh = cfg->iou_thresh; a.max_age = cfg->max_age; a.refresh = cfg->refresh; a.retry = cfg->retry;
    a.B = B; a.cap = cap; a.T = trk->T;
    hipLaunchKernelGGL(track_walk, dim3(trk->S), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(track_pack, dim3(cdiv(B + 1, 4)), dim3(256), 0, ctx->stream, a.tab, a.nemb, counts_dev, track_dev, B, cap, offsets_dev,
                       src_dev, row_cap);
    FID_HIP(hipGetLastError());
    trk->pending = true;
    trk->serial += 1;
    trk->B = B; trk->cap = cap; trk->row_cap = row_cap;
    trk->stream.assign(stream, stream + B);
    return FID_OK;
}

int fid_track_identify(fid_ctx *ctx, fid_tracker *trk, const int32_t *counts_dev, const int32_t *stream, int B, int cap,
                       const int32_t *track_dev, const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, const int32_t *idx_dev,
                       const float *score_dev, int n_rows, int32_t *ident_idx_dev, float *ident_score_dev) {
    FID_REQUIRE(ctx && trk && counts_dev && stream && track_dev && offsets_dev && src_dev && ident_idx_dev && ident_score_dev,
                "track identify: NULL argument");
    FID_TRY(check_shape(stream, B, cap, row_cap, trk->S));
    FID_REQUIRE(n_rows >= 0 && n_rows <= row_cap, "track identify: n_rows %d outside [0, row_cap = %d]", n_rows, row_cap);
    FID_REQUIRE(n_rows == 0 || (idx_dev && score_dev), "track identify: NULL idx / score with n_rows %d", n_rows);
    FID_REQUIRE(trk->pending, "track identify: no fid_track_step is pending");
    FID_REQUIRE(B == trk->B && cap == trk->cap && row_cap == trk->row_cap && memcmp(stream, trk->stream.data(), (size_t)B * 4) == 0,
                "track identify: B, cap, row_cap or the stream array differ from the pending fid_track_step's");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    IdentArgs a{};
    a.slots = trk->slots; a.tab = trk->tab;   // (the table the step stored: nobody else writes it)
    a.counts = counts_dev; a.track = track_dev; a.offsets = offsets_dev; a.idx = idx_dev; a.score = score_dev;
    a.out_idx = ident_idx_dev; a.out_score = ident_score_dev;
    a.n_rows = n_rows; a.B = B; a.cap = cap; a.S = trk->S; a.T = trk->T;
    hipLaunchKernelGGL(track_identify, dim3(trk->S), dim3(64), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    trk->pending = false;
    return FID_OK;
}

}  // extern "C"
