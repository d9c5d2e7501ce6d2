// Coasting tracks through the frames where the detector missed them (include/faceid.h: fid_coaster_*, fid_track_coast).  The coaster follows
// the tracker: per (stream, slot) it remembers the track's last box, its velocity, its detection score and its name, and for every frame of
// a step it emits the tracks that are alive but took no detection in that frame, behind the frame's detections, in tables the draw and
// redact kernels read unchanged.  (No reference analogue: the reference draws what it detects, main.py:130-148.)
//
// State (S x T entries of 16 words) lives in device memory.  One call is two launches, ordered by the context's stream only -- no workgroup
// waits for another, nothing is polled, no LDS, no barrier, no atomics:
//
//   coast_walk    track_walk's shape: one wave64 per stream, lane l owns entry l in registers (loaded once, stored once).  The stream's
//                 frames are visited in batch order; a frame's {id, word}, box, conf and identity are loaded 64 detections at a time (one per
//                 lane).  Each lane learns the HIGHEST detection of the frame that names its slot -- the slot words go from lane to lane
//                 through v_readlane, tracked detections only -- and fetches that one detection's words from the lane that loaded it.  At
//                 the end of the frame a lane either took a detection or ages, and writes one staging record -- coasted flag, id, missed,
//                 identity, conf, emitted box -- into a [B][T] table in the context's scratch, with plain vector stores.
//   coast_merge   one workgroup per frame: the frame's k_b rows of the four inputs are copied, its T staging records are compacted in slot
//                 order behind them (ballot + popcount: track_pack's idiom) and the fillers written behind those.  Every wave of the
//                 workgroup reads the T flags itself, so nobody waits for the count.  Inside the launch no two workgroups write one
//                 destination: a frame's rows belong to its workgroup.
//
// A skipped frame has no staging records; the merge never reads them.  The frame-to-stream table is the one the tracker's last step stored
// (track_state.h): nobody writes it before the next step.
//
// This file must never get a fast-math flag: velocity, prediction and growth (coast_core.h) round every fp32 operation on its own, with the
// correctly rounded divide and no FMA, and are compared bit for bit with the host twin and a numpy restatement.
#include "common.h"
#include "coast_core.h"
#include "track_state.h"

struct fid_coaster {
    int S = 0, T = 0, device = 0;
    int32_t *entries = nullptr;                              // [S*T][16]
    const fid_tracker *last_trk = nullptr;                   // the step the last coast followed
    unsigned long long last_serial = 0;
};

namespace {

using fid::cdiv;

constexpr int CW = FID_COAST_WORDS;
constexpr int STW = 12;                                      // staging record: coasted, id, missed, ident_idx | ident_score, conf, x1, y1 | x2, y2, 0, 0
static_assert(CW == 16, "entries are moved as four 16-byte vectors");

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__device__ __forceinline__ void entry_load(fid_coast_entry &e, const int32_t *w) {
    const int4 a = ((const int4 *)w)[0], b = ((const int4 *)w)[1], c = ((const int4 *)w)[2], d = ((const int4 *)w)[3];
    e.id = a.x; e.missed = a.y; e.has_vel = a.z; e.ident_idx = a.w; e.ident_score = b.x;
    e.box[0] = __int_as_float(b.y); e.box[1] = __int_as_float(b.z); e.box[2] = __int_as_float(b.w); e.box[3] = __int_as_float(c.x);
    e.vel[0] = __int_as_float(c.y); e.vel[1] = __int_as_float(c.z); e.vel[2] = __int_as_float(c.w); e.vel[3] = __int_as_float(d.x);
    e.conf = __int_as_float(d.y);
}
__device__ __forceinline__ void entry_store(const fid_coast_entry &e, int32_t *w) {
    ((int4 *)w)[0] = make_int4(e.id, e.missed, e.has_vel, e.ident_idx);
    ((int4 *)w)[1] = make_int4(e.ident_score, fid_coast_bits(e.box[0]), fid_coast_bits(e.box[1]), fid_coast_bits(e.box[2]));
    ((int4 *)w)[2] = make_int4(fid_coast_bits(e.box[3]), fid_coast_bits(e.vel[0]), fid_coast_bits(e.vel[1]), fid_coast_bits(e.vel[2]));
    ((int4 *)w)[3] = make_int4(fid_coast_bits(e.vel[3]), fid_coast_bits(e.conf), 0, 0);
}

struct WalkArgs {
    int32_t *entries, *stage;                                // [S*T][16], [B][T][12]
    const int32_t *tab;                                      // [B] stream of frame b (the tracker's)
    const float *det;
    const int32_t *counts, *track;
    const int32_t *ident_idx;                                // may both be NULL
    const float *ident_score;
    fid_coast_config cfg;
    int B, cap, T;
};

__global__ void __launch_bounds__(64) coast_walk(const WalkArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < a.T;
    int32_t *w = a.entries + ((size_t)s * a.T + (mine ? lane : 0)) * CW;
    fid_coast_entry e;
    fid_coast_entry_clear(e);
    if (mine) entry_load(e, w);
    // One wave is alone with the latency of every load it waits for: the frames' table entries and the detections' words come 64 at a
    // time, one per lane.
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int nb = min(64, a.B - b0);
        int f_stream = -1, f_k = 0;
        if (lane < nb) { f_stream = a.tab[b0 + lane]; f_k = min(max(a.counts[b0 + lane], 0), a.cap); }
        for (int jb = 0; jb < nb; jb++) {
            if (lane_i(f_stream, jb) != s) continue;         // (wave-uniform)
            const int b = b0 + jb, k = lane_i(f_k, jb);
            bool have = false;                               // this lane's slot is named by a detection of the frame: the highest one's words
            int c_id = -1, c_word = -1, c_ii = -1, c_is = 0;
            float c_d[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int f0 = 0; f0 < k; f0 += 64) {
                const int n = min(64, k - f0);
                int tid = -1, word = -1, r_ii = -1, r_is = 0;
                float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, d4 = 0.f;
                if (lane < n) {
                    const size_t face = (size_t)b * a.cap + f0 + lane;
                    const int2 t = *(const int2 *)(a.track + face * 2);
                    const float *d = a.det + face * 5;
                    tid = t.x; word = t.y;
                    d0 = d[0]; d1 = d[1]; d2 = d[2]; d3 = d[3]; d4 = d[4];
                    if (a.ident_idx) { r_ii = a.ident_idx[face]; r_is = __float_as_int(a.ident_score[face]); }
                }
                const int slot = fid_coast_slot(tid, word, a.T);                 // -1: untracked, or no detection in this lane
                int pick = -1;
                unsigned long long work = __ballot(slot >= 0);
                while (work != 0ull) {                       // (wave-uniform) ascending: a slot named twice keeps the higher detection
                    const int j = __ffsll((long long)work) - 1;
                    work &= work - 1ull;
                    if (lane == lane_i(slot, j)) pick = j;
                }
                if (__ballot(pick >= 0) != 0ull) {           // (wave-uniform, and only lanes < T can have picked)
                    const int from = pick >= 0 ? pick : lane;
                    const int t_id = __shfl(tid, from), t_word = __shfl(word, from), t_ii = __shfl(r_ii, from), t_is = __shfl(r_is, from);
                    const float t0 = __shfl(d0, from), t1 = __shfl(d1, from), t2 = __shfl(d2, from), t3 = __shfl(d3, from), t4 = __shfl(d4, from);
                    if (pick >= 0) {
                        have = true;
                        c_id = t_id; c_word = t_word; c_ii = t_ii; c_is = t_is;
                        c_d[0] = t0; c_d[1] = t1; c_d[2] = t2; c_d[3] = t3; c_d[4] = t4;
                    }
                }
            }
            if (mine) {                                      // end of frame
                float box[4] = {0.f, 0.f, 0.f, 0.f};
                bool coasts = false;
                if (have) fid_coast_take(e, c_id, c_word, c_d, c_ii, c_is);
                else if (e.id >= 0) coasts = fid_coast_age(e, a.cfg, box);
                int4 *rec = (int4 *)(a.stage + ((size_t)b * a.T + lane) * STW);
                rec[0] = make_int4(coasts ? 1 : 0, e.id, e.missed, e.ident_idx);
                rec[1] = make_int4(e.ident_score, fid_coast_bits(e.conf), __float_as_int(box[0]), __float_as_int(box[1]));
                rec[2] = make_int4(__float_as_int(box[2]), __float_as_int(box[3]), 0, 0);
            }
        }
    }
    if (mine) entry_store(e, w);
}

struct MergeArgs {
    const int32_t *stage, *tab;
    const int32_t *det, *counts, *track, *ident_idx, *ident_score;               // (floats are moved as their words)
    int32_t *det_out, *counts_out, *track_out, *idx_out, *score_out;
    int B, cap, T;
};

// workgroup b: frame b
__global__ void __launch_bounds__(256) coast_merge(const MergeArgs a) {
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int cap2 = a.cap + a.T;
    const bool live = a.tab[b] >= 0;
    const int k = live ? min(max(a.counts[b], 0), a.cap) : 0;
    const size_t in0 = (size_t)b * a.cap, out0 = (size_t)b * cap2;
    for (int i = t; i < k * 5; i += 256) a.det_out[out0 * 5 + i] = a.det[in0 * 5 + i];
    for (int i = t; i < k; i += 256) {
        *(int2 *)(a.track_out + (out0 + i) * 2) = *(const int2 *)(a.track + (in0 + i) * 2);
        a.idx_out[out0 + i] = a.ident_idx ? a.ident_idx[in0 + i] : -1;
        a.score_out[out0 + i] = a.ident_score ? a.ident_score[in0 + i] : 0;
    }
    const int32_t *rec = a.stage + ((size_t)b * a.T + (lane < a.T ? lane : 0)) * STW;
    const bool flag = live && lane < a.T && rec[0] != 0;
    const unsigned long long m = __ballot(flag);             // (the same in every wave of the workgroup)
    const int n = k + __popcll(m);
    if (t < 64 && flag) {
        const int4 r0 = ((const int4 *)rec)[0], r1 = ((const int4 *)rec)[1];
        const int2 r2 = ((const int2 *)rec)[4];
        const size_t at = out0 + k + lanes_below(m, lane);
        int32_t *d = a.det_out + at * 5;
        d[0] = r1.z; d[1] = r1.w; d[2] = r2.x; d[3] = r2.y; d[4] = r1.y;
        *(int2 *)(a.track_out + at * 2) = make_int2(r0.y, lane | FID_TRACK_COASTED | (r0.z << 16));
        a.idx_out[at] = r0.w;
        a.score_out[at] = r1.x;
    }
    if (t == 0) a.counts_out[b] = n;
    for (int i = n + t; i < cap2; i += 256) {
        int32_t *d = a.det_out + (out0 + i) * 5;
        d[0] = d[1] = d[2] = d[3] = d[4] = 0;
        *(int2 *)(a.track_out + (out0 + i) * 2) = make_int2(-1, -1);
        a.idx_out[out0 + i] = -1;
        a.score_out[out0 + i] = 0;
    }
}

// the entries of stream `which` (-1: of every stream) become free
__global__ void __launch_bounds__(256) coast_reset(int32_t *entries, int n_entries, int T, int which) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_entries * CW) return;
    if (which < 0 || gid / CW / T == which) entries[gid] = gid % CW == 0 ? -1 : 0;
}

}  // namespace

extern "C" {

int fid_coaster_create(fid_ctx *ctx, int S, int T, fid_coaster **out) {
    FID_REQUIRE(ctx && out, "coaster: NULL argument");
    FID_REQUIRE(S >= 1 && (long long)S * FID_TRACK_MAX_SLOTS * CW <= 0x7FFFFFFFll, "coaster: %d streams", S);
    FID_REQUIRE(T >= 1 && T <= FID_TRACK_MAX_SLOTS, "coaster: %d slots per stream (1 .. %d)", T, FID_TRACK_MAX_SLOTS);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    fid_coaster *c = new fid_coaster();
    c->S = S; c->T = T; c->device = ctx->device;
    if (hipMalloc((void **)&c->entries, (size_t)S * T * CW * 4) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        fid::set_error("coaster: out of device memory for %d x %d entries", S, T);
        return FID_E_NOMEM;
    }
    hipLaunchKernelGGL(coast_reset, dim3(cdiv(S * T * CW, 256)), dim3(256), 0, ctx->stream, c->entries, S * T, T, -1);
    FID_HIP(hipGetLastError());
    *out = c;
    return FID_OK;
}

int fid_coaster_destroy(fid_ctx *ctx, fid_coaster *c) {
    FID_REQUIRE(ctx, "coaster: NULL context");
    if (!c) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    if (c->entries) (void)hipFree(c->entries);
    delete c;
    return FID_OK;
}

int fid_coaster_reset(fid_ctx *ctx, fid_coaster *c, int stream) {
    FID_REQUIRE(ctx && c, "coaster reset: NULL argument");
    FID_REQUIRE(stream >= -1 && stream < c->S, "coaster reset: stream %d, the coaster has %d", stream, c->S);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(coast_reset, dim3(cdiv(c->S * c->T * CW, 256)), dim3(256), 0, ctx->stream, c->entries, c->S * c->T, c->T, stream);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_coaster_read(fid_ctx *ctx, fid_coaster *c, int32_t *entries_host) {
    FID_REQUIRE(ctx && c && entries_host, "coaster read: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipMemcpyAsync(entries_host, c->entries, (size_t)c->S * c->T * CW * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    return FID_OK;
}

int fid_track_coast(fid_ctx *ctx, fid_coaster *c, fid_tracker *trk, const int32_t *stream, int B, int cap, const float *det_dev,
                    const int32_t *counts_dev, const int32_t *track_dev, const int32_t *ident_idx_dev, const float *ident_score_dev,
                    const fid_coast_config *cfg, float *det_out, int32_t *counts_out, int32_t *track_out, int32_t *idx_out, float *score_out) {
    FID_REQUIRE(ctx && c && trk, "track coast: NULL argument");
    const char *why = fid_coast_check(c->S, c->T, stream, B, cap, det_dev, counts_dev, track_dev, ident_idx_dev, ident_score_dev, cfg, det_out,
                                      counts_out, track_out, idx_out, score_out);
    FID_REQUIRE(why == nullptr, "track coast: %s", why ? why : "");
    FID_REQUIRE(c->S == trk->S && c->T == trk->T, "track coast: the coaster has %d x %d entries, the tracker %d x %d slots", c->S, c->T, trk->S,
                trk->T);
    FID_REQUIRE(!trk->pending, "track coast: the step's fid_track_identify has not been called");
    FID_REQUIRE(trk->serial > 0, "track coast: the tracker has not run a step");
    FID_REQUIRE(B == trk->B && cap == trk->cap && memcmp(stream, trk->stream.data(), (size_t)B * 4) == 0,
                "track coast: B, cap or the stream array differ from the tracker's last step's");
    FID_REQUIRE(!(c->last_trk == trk && c->last_serial == trk->serial), "track coast: this step has been coasted already");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    void *ws;
    FID_TRY(fid::get_scratch(ctx, 2, (size_t)B * c->T * STW * 4, &ws));
    WalkArgs a{};
    a.entries = c->entries; a.stage = (int32_t *)ws; a.tab = trk->tab;
    a.det = det_dev; a.counts = counts_dev; a.track = track_dev; a.ident_idx = ident_idx_dev; a.ident_score = ident_score_dev;
    a.cfg = *cfg; a.B = B; a.cap = cap; a.T = c->T;
    MergeArgs m{};
    m.stage = (const int32_t *)ws; m.tab = trk->tab;
    m.det = (const int32_t *)det_dev; m.counts = counts_dev; m.track = track_dev; m.ident_idx = ident_idx_dev;
    m.ident_score = (const int32_t *)ident_score_dev;
    m.det_out = (int32_t *)det_out; m.counts_out = counts_out; m.track_out = track_out; m.idx_out = idx_out; m.score_out = (int32_t *)score_out;
    m.B = B; m.cap = cap; m.T = c->T;
    hipLaunchKernelGGL(coast_walk, dim3(c->S), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(coast_merge, dim3(B), dim3(256), 0, ctx->stream, m);
    FID_HIP(hipGetLastError());
    c->last_trk = trk;
    c->last_serial = trk->serial;
    return FID_OK;
}

int fid_track_coast_host(int32_t *entries, int S, int T, const int32_t *stream, int B, int cap, const float *det, const int32_t *counts,
                         const int32_t *track, const int32_t *ident_idx, const float *ident_score, const fid_coast_config *cfg, float *det_out,
                         int32_t *counts_out, int32_t *track_out, int32_t *idx_out, float *score_out) {
    FID_REQUIRE(entries, "track coast: NULL entries");
    const char *why = fid_coast_check(S, T, stream, B, cap, det, counts, track, ident_idx, ident_score, cfg, det_out, counts_out, track_out,
                                      idx_out, score_out);
    FID_REQUIRE(why == nullptr, "track coast: %s", why ? why : "");
    fid_track_coast_table_host(entries, S, T, stream, B, cap, det, counts, track, ident_idx, ident_score, cfg, det_out, counts_out, track_out,
                               idx_out, score_out);
    return FID_OK;
}

}  // extern "C"
