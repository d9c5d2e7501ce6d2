// Best shots of the tracker's tracks, kept on the device, and ended tracks handed out as visits (include/faceid.h: fid_shot_score, fid_shots_*,
// fid_track_keep).  Among the faces a track embeds, the keeper holds the one with the highest score -- its unit embedding, its aligned crop and
// where it came from -- and when the track ends that one record moves to the finished store, ready for fid_gallery_group where it lies.  (No
// reference analogue: the reference embeds every face of every frame and keeps a per-visit image on disk, smart_face_recognition.py.)
//
// State (S x T live entries, finished_cap finished records, a frame counter per stream) lives in device memory.  One keep is three launches,
// ordered by the context's stream only -- no workgroup waits for another, nothing is polled, no LDS, no atomics:
//
//   shot_walk            track_walk's shape: one wave64 per stream, lane l owns live entry l in registers (loaded once, stored once).  The
//                        stream's frames are visited in batch order, a frame's rows are loaded 64 at a time (one per lane) and handed lane to
//                        lane.  The walk DECIDES and writes meta words only; it moves no payload.  What it decides goes into an event table:
//                        a record that finishes -- its meta, where its payload lies (a live entry, or a row of this step when the shot was
//                        taken in this very call) and its ordinal among the stream's finished records (a wave-uniform counter: the order of
//                        the rules) -- and, per live entry, the one row of this step whose payload it must hold afterwards.  A finish caused
//                        by row i sits at event i, one caused by the closing slot walk at event n_rows + s * T + slot: the host cannot know
//                        how many there are without a read-back, so the grid of the copies is this upper bound either way, and a table
//                        indexed by cause needs no compaction.  Events carry the call's serial: a stale one is never taken for a fresh one.
//   shot_copy_finished   one workgroup per event: finished index = count + finished records of the streams before (every workgroup sums the
//                        per-stream counts before its stream: track_pack's idiom) + ordinal; beyond finished_cap the record is dropped.
//   shot_copy_live       one workgroup per live entry: the row it must hold -> the live store.  Workgroup 0 also advances count / dropped.
//
// The order of the two copy launches is the point: a slot whose old shot finishes while its new track's row is stored in the same call has
// its old payload read (launch 2) before it is overwritten (launch 3).  Inside one launch no two workgroups write one destination: the walk
// emits at most one store per live entry and call, and finished indices are distinct.
//
// This file must never get a fast-math flag: the score (shot_core.h) rounds every operation on its own, with the correctly rounded divide,
// and is compared bit for bit with its host twin and a numpy restatement.
#include "common.h"
#include "shot_core.h"
#include "track_state.h"

struct fid_shots {
    int S = 0, T = 0, dim = 0, cap = 0, keep_crops = 0, device = 0;
    int32_t *live_meta = nullptr, *fin_meta = nullptr;       // [S*T][16], [cap][16]
    uint16_t *live_q = nullptr, *fin_q = nullptr;            // [..][dim]
    uint8_t *live_crop = nullptr, *fin_crop = nullptr;       // [..][112*112*3] (keep_crops)
    int32_t *counters = nullptr;                             // [2] = {count, dropped} | [S] frames | [S] finished by the last walk | [S*T] live events
    int32_t *ev = nullptr;                                   // [ev_rows + S*T][EVW]
    int ev_rows = 0;
    std::vector<void *> retired;                             // outgrown event tables: freed with the handle, so growing never synchronises
    const fid_tracker *last_trk = nullptr;                   // the step the last keep followed
    unsigned long long last_serial = 0;
    int launches = 0;                                        // serial of the event table's writer
};

namespace {

using fid::cdiv;

constexpr int SW = FID_TRACK_SLOT_WORDS;
constexpr int MW = FID_SHOT_META_WORDS;
constexpr int EVW = 20;                                      // event: stream (-1: none), ordinal, source, serial, meta[16]
constexpr int CROP_BYTES = 112 * 112 * 3;                    // 37 632 = 2 352 x 16
static_assert(MW == 16 && CROP_BYTES % 16 == 0, "records are moved as 16-byte vectors");

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(lane_i(__float_as_int(v), l)); }
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// one live entry in registers: meta words 1 .. 11 (word 0 is the stream, 12 .. 15 are 0)
struct Entry {
    int id, ii, is, frame, rows, b0, b1, b2, b3, dsc;
    float sc;                                                // -1: no shot yet
};

__device__ __forceinline__ void entry_clear(Entry &e) {
    e.id = -1; e.ii = e.is = e.frame = e.rows = e.b0 = e.b1 = e.b2 = e.b3 = e.dsc = 0; e.sc = 0.f;
}
__device__ __forceinline__ void entry_begin(Entry &e, int id) {
    entry_clear(e);
    e.id = id; e.ii = -1; e.sc = -1.0f;
}
__device__ __forceinline__ void entry_load(Entry &e, const int32_t *m) {
    const int4 a = ((const int4 *)m)[0], b = ((const int4 *)m)[1], c = ((const int4 *)m)[2];
    e.id = a.y; e.ii = a.z; e.is = a.w; e.sc = __int_as_float(b.x); e.frame = b.y; e.rows = b.z; e.b0 = b.w;
    e.b1 = c.x; e.b2 = c.y; e.b3 = c.z; e.dsc = c.w;
}
// meta[16] of the entry as stream s holds it (an empty entry: -1 in word 1, 0 elsewhere)
__device__ __forceinline__ void entry_store(const Entry &e, int s, int32_t *m) {
    const bool live = e.id != -1;
    ((int4 *)m)[0] = make_int4(live ? s : 0, e.id, e.ii, e.is);
    ((int4 *)m)[1] = make_int4(__float_as_int(e.sc), e.frame, e.rows, e.b0);
    ((int4 *)m)[2] = make_int4(e.b1, e.b2, e.b3, e.dsc);
    ((int4 *)m)[3] = make_int4(0, 0, 0, 0);
}
// the entry finishes as the stream's record `ordinal`; its payload lies in live entry `entry`, or in row `row` of this step when row >= 0
__device__ __forceinline__ void event_store(int32_t *ev, const Entry &e, int s, int ordinal, int entry, int row, int serial) {
    ((int4 *)ev)[0] = make_int4(s, ordinal, row >= 0 ? ~row : entry, serial);
    entry_store(e, s, ev + 4);
}

struct KeepArgs {
    int32_t *live_meta, *frames, *nfin, *live_ev, *ev;
    const int32_t *slots, *tab;                              // the tracker's slots (word 0: the id a slot holds now) and its stream table [B]
    const int32_t *track, *offsets, *src;
    const float *score, *det;
    const int32_t *ident_idx;                                // may both be NULL
    const float *ident_score;
    int n_rows, B, cap, T, serial;                           // n_rows: already min(n_rows, row_cap)
};

__global__ void __launch_bounds__(64) shot_walk(const KeepArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < a.T;
    const int entry = s * a.T + (mine ? lane : 0);
    Entry e;
    entry_clear(e);
    if (mine) entry_load(e, a.live_meta + (size_t)entry * MW);
    int cur = -1;                                            // the row of this step that holds the entry's shot; -1: the live store does
    int frame_no = a.frames[s], nfin = 0;                    // (the same in every lane)
    const int total = min(max(a.offsets[a.B], 0), a.n_rows);
    const int faces = a.B * a.cap;
    // One wave is alone with the latency of every load it waits for, so nothing is loaded per frame or per row: the frames' table entries
    // and the rows' words come 64 at a time, one per lane, and go from lane to lane through v_readlane.
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int nb = min(64, a.B - b0);
        int f_stream = -1, f_lo = 0, f_hi = 0;
        if (lane < nb) { f_stream = a.tab[b0 + lane]; f_lo = a.offsets[b0 + lane]; f_hi = a.offsets[b0 + lane + 1]; }
        for (int jb = 0; jb < nb; jb++) {
            if (lane_i(f_stream, jb) != s) continue;         // (wave-uniform)
            const int r1 = min(lane_i(f_hi, jb), total);
            for (int i0 = max(lane_i(f_lo, jb), 0); i0 < r1; i0 += 64) {
                const int n = min(64, r1 - i0);
                int tid = -1, word = -1, r_ii = -1, r_is = 0, d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0;
                float rsc = -1.f;
                if (lane < n) {
                    const int face = a.src[i0 + lane];
                    rsc = a.score[i0 + lane];
                    if (face >= 0 && face < faces) {
                        const int2 t = *(const int2 *)(a.track + (size_t)face * 2);
                        const int32_t *d = (const int32_t *)a.det + (size_t)face * 5;
                        tid = t.x; word = t.y;
                        d0 = d[0]; d1 = d[1]; d2 = d[2]; d3 = d[3]; d4 = d[4];
                        if (a.ident_idx) { r_ii = a.ident_idx[face]; r_is = __float_as_int(a.ident_score[face]); }
                    }
                }
                for (int j = 0; j < n; j++) {
                    const int w = lane_i(word, j), t = lane_i(tid, j);
                    int32_t *ev = a.ev + (size_t)(i0 + j) * EVW;
                    if (w < 0 || t < 0 || (w & 63) >= a.T) { // an untracked face (wave-uniform)
                        if (lane == 0) ev[0] = -1;
                        continue;
                    }
                    const int slot = w & 63;
                    const float sc = lane_f(rsc, j);
                    const int ii = lane_i(r_ii, j), is = lane_i(r_is, j);
                    const int x0 = lane_i(d0, j), x1 = lane_i(d1, j), x2 = lane_i(d2, j), x3 = lane_i(d3, j), x4 = lane_i(d4, j);
                    // the slot holds another track now -- another id, or a track that STARTS with this row under the same id (after a
                    // tracker reset the ids begin again at 0) --: the old one finishes
                    const bool ends = lane == slot && e.id != -1 && (e.id != t || (w & FID_TRACK_STARTED) != 0);
                    const bool record = ends && e.sc >= 0.f;                     // ... with a record if it ever had a candidate
                    const bool any = __ballot(record) != 0ull;
                    if (lane == slot) {
                        if (record) event_store(ev, e, s, nfin, entry, cur, a.serial);
                        else ev[0] = -1;
                        if (ends || e.id == -1) { entry_begin(e, t); cur = -1; }
                        e.rows += 1;
                        if (a.ident_idx) { e.ii = ii; e.is = is; }
                        if (sc >= 0.f && (!(e.sc >= 0.f) || sc > e.sc)) {        // strict: the earlier row stays on a tie; false for a NaN
                            e.sc = sc; e.frame = frame_no;
                            e.b0 = x0; e.b1 = x1; e.b2 = x2; e.b3 = x3; e.dsc = x4;
                            cur = i0 + j;
                        }
                    }
                    nfin += any ? 1 : 0;
                }
            }
            frame_no += 1;
        }
    }
    // slots in ascending order: an entry whose track the tracker's slot no longer holds (freed, reset, reused without a row) finishes
    const int now = mine ? a.slots[(size_t)entry * SW] : -1;
    const bool ends = mine && e.id != -1 && e.id != now;
    const bool record = ends && e.sc >= 0.f;
    const unsigned long long rec = __ballot(record);
    if (mine) {
        int32_t *ev = a.ev + ((size_t)a.n_rows + entry) * EVW;
        if (record) event_store(ev, e, s, nfin + lanes_below(rec, lane), entry, cur, a.serial);
        else ev[0] = -1;
        if (ends) { entry_clear(e); cur = -1; }
        a.live_ev[entry] = cur;
        entry_store(e, s, a.live_meta + (size_t)entry * MW);
    }
    nfin += __popcll(rec);
    if (lane == 0) { a.frames[s] = frame_no; a.nfin[s] = nfin; }
}

// every live entry of stream `which` (-1: of every stream) finishes, in slot order
__global__ void __launch_bounds__(64) shot_flush(int32_t *live_meta, int32_t *nfin, int32_t *live_ev, int32_t *evt, int T, int which, int serial) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < T;
    const int entry = s * T + (mine ? lane : 0);
    Entry e;
    entry_clear(e);
    if (mine) entry_load(e, live_meta + (size_t)entry * MW);
    const bool ends = mine && (which < 0 || which == s) && e.id != -1;
    const bool record = ends && e.sc >= 0.f;
    const unsigned long long rec = __ballot(record);
    if (mine) {
        int32_t *ev = evt + (size_t)entry * EVW;
        if (record) event_store(ev, e, s, lanes_below(rec, lane), entry, -1, serial);
        else ev[0] = -1;
        live_ev[entry] = -1;
        if (ends) {
            entry_clear(e);
            entry_store(e, s, live_meta + (size_t)entry * MW);
        }
    }
    if (lane == 0) nfin[s] = __popcll(rec);
}

__global__ void __launch_bounds__(256) shot_reset(int32_t *live_meta, int n_entries, int32_t *counters, int n_counters) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < n_entries * MW) live_meta[gid] = gid % MW == 1 ? -1 : 0;
    if (gid < n_counters) counters[gid] = 0;
}

__global__ void __launch_bounds__(64) shot_clear_finished(int32_t *counters) {
    if (threadIdx.x == 0) *(int2 *)counters = make_int2(0, 0);
}

// one record's payload, by the whole workgroup.  The stores' rows are 16-byte aligned where their size allows; a caller's pointer need not be.
__device__ void copy_q(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int dim) {
    if ((dim & 7) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0u) {
        for (int i = threadIdx.x; i < dim / 8; i += 256) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    } else {
        for (int i = threadIdx.x; i < dim; i += 256) dst[i] = src[i];
    }
}
__device__ void copy_crop(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst) {       // dst: a store's row, 16-byte aligned
    if (((uintptr_t)src & 15u) == 0u) {
        for (int i = threadIdx.x; i < CROP_BYTES / 16; i += 256) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    } else {
        for (int i = threadIdx.x; i < CROP_BYTES / 16; i += 256) {
            const uint8_t *p = src + (size_t)i * 16;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
            ((uint4 *)dst)[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

struct CopyArgs {
    const int32_t *ev, *nfin, *live_ev, *offsets;            // offsets: NULL for a flush (no row events)
    int32_t *counters;                                       // {count, dropped}
    int32_t *fin_meta;
    uint16_t *fin_q, *live_q;
    uint8_t *fin_crop, *live_crop;                           // NULL without crops
    const uint16_t *q;                                       // the step's rows
    const uint8_t *crops;
    int n_rows, B, S, T, dim, cap, serial;
};

// workgroup g: event g.  Row events beyond the step's rows and events of another call are not events.
__global__ void __launch_bounds__(256) shot_copy_finished(const CopyArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x & 63;
    if (g < a.n_rows && g >= min(max(a.offsets[a.B], 0), a.n_rows)) return;
    const int32_t *ev = a.ev + (size_t)g * EVW;
    const int4 head = *(const int4 *)ev;                     // stream, ordinal, source, serial
    if (head.x < 0 || head.x >= a.S || head.w != a.serial) return;
    int before = 0;                                          // finished records of the streams before this one (<= n_rows + S * T: fits an int)
    for (int s0 = 0; s0 < head.x; s0 += 64) before += s0 + lane < head.x ? a.nfin[s0 + lane] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    const long long at = (long long)a.counters[0] + before + head.y;
    if (at >= a.cap) return;                                 // the finished store is full: dropped (shot_copy_live counts it)
    if (threadIdx.x < MW) a.fin_meta[(size_t)at * MW + threadIdx.x] = ev[4 + threadIdx.x];
    const bool from_row = head.z < 0;
    const size_t from = from_row ? (size_t)~head.z : (size_t)head.z;
    copy_q((from_row ? a.q : a.live_q) + from * a.dim, a.fin_q + (size_t)at * a.dim, a.dim);
    if (a.fin_crop) copy_crop((from_row ? a.crops : a.live_crop) + from * CROP_BYTES, a.fin_crop + (size_t)at * CROP_BYTES);
}

// workgroup e: live entry e takes the payload of the row the walk named.  Workgroup 0, wave 0: count and dropped.
__global__ void __launch_bounds__(256) shot_copy_live(const CopyArgs a) {
    const int e = blockIdx.x;
    if (e == 0 && threadIdx.x < 64) {
        long long total = 0;
        for (int s0 = 0; s0 < a.S; s0 += 64) total += s0 + (int)threadIdx.x < a.S ? a.nfin[s0 + threadIdx.x] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        if (threadIdx.x == 0) {
            const long long want = (long long)a.counters[0] + total, count = want < a.cap ? want : a.cap;
            *(int2 *)a.counters = make_int2((int)count, (int)((long long)a.counters[1] + (want - count)));
        }
    }
    const int row = a.live_ev[e];
    if (row < 0 || row >= a.n_rows) return;
    copy_q(a.q + (size_t)row * a.dim, a.live_q + (size_t)e * a.dim, a.dim);
    if (a.live_crop) copy_crop(a.crops + (size_t)row * CROP_BYTES, a.live_crop + (size_t)e * CROP_BYTES);
}

__global__ void __launch_bounds__(256) shot_score(const int64_t *__restrict__ stats, const float *__restrict__ measure, int n_rows, float n_s,
                                                  float n_c, float n_r, float *__restrict__ score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_rows) score[i] = fid_shot_score_row(stats[(size_t)i * 8 + 7], measure + (size_t)i * 8, n_s, n_c, n_r);
}

// the event table holds `rows` row events and the S * T slot events
int ev_reserve(fid_shots *sh, int rows) {
    if (sh->ev && sh->ev_rows >= rows) return FID_OK;
    const int want = std::max(1024, rows + rows / 4);
    int32_t *p = nullptr;
    if (hipMalloc((void **)&p, ((size_t)want + (size_t)sh->S * sh->T) * EVW * 4) != hipSuccess) {
        fid::set_error("shots: out of device memory for %d events", want);
        return FID_E_NOMEM;
    }
    if (sh->ev) sh->retired.push_back(sh->ev);               // (work that is still queued may read it)
    sh->ev = p;
    sh->ev_rows = want;
    return FID_OK;
}

void free_all(fid_shots *sh) {
    for (void *p : {(void *)sh->live_meta, (void *)sh->fin_meta, (void *)sh->live_q, (void *)sh->fin_q, (void *)sh->live_crop,
                    (void *)sh->fin_crop, (void *)sh->counters, (void *)sh->ev})
        if (p) (void)hipFree(p);
    for (void *p : sh->retired) (void)hipFree(p);
    delete sh;
}

CopyArgs copy_args(const fid_shots *sh) {
    CopyArgs c{};
    c.ev = sh->ev; c.counters = sh->counters; c.nfin = sh->counters + 2 + sh->S; c.live_ev = sh->counters + 2 + 2 * sh->S;
    c.fin_meta = sh->fin_meta; c.fin_q = sh->fin_q; c.live_q = sh->live_q; c.fin_crop = sh->fin_crop; c.live_crop = sh->live_crop;
    c.S = sh->S; c.T = sh->T; c.dim = sh->dim; c.cap = sh->cap;
    return c;
}

}  // namespace

extern "C" {

int fid_shot_score(fid_ctx *ctx, const int64_t *stats_dev, const float *measure_dev, int n_rows, const fid_measure_config *mcfg,
                   float *score_dev) {
    FID_REQUIRE(ctx, "shot score: NULL context");
    const char *why = fid_shot_score_check(stats_dev, measure_dev, n_rows, mcfg, score_dev);
    FID_REQUIRE(why == nullptr, "shot score: %s", why ? why : "");
    if (n_rows == 0) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(shot_score, dim3(cdiv(n_rows, 256)), dim3(256), 0, ctx->stream, stats_dev, measure_dev, n_rows,
                       mcfg->sharpness_normalization, mcfg->contrast_normalization, mcfg->residual_normalization, score_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_shot_score_host(const int64_t *stats, const float *measure, int n_rows, const fid_measure_config *mcfg, float *score) {
    const char *why = fid_shot_score_check(stats, measure, n_rows, mcfg, score);
    FID_REQUIRE(why == nullptr, "shot score: %s", why ? why : "");
    fid_shot_score_table_host(stats, measure, n_rows, mcfg, score);
    return FID_OK;
}

int fid_shots_create(fid_ctx *ctx, int S, int T, int dim, int finished_cap, int keep_crops, fid_shots **out) {
    FID_REQUIRE(ctx && out, "shots: NULL argument");
    FID_REQUIRE(S >= 1 && (long long)S * FID_TRACK_MAX_SLOTS * MW <= 0x7FFFFFFFll, "shots: %d streams", S);
    FID_REQUIRE(T >= 1 && T <= FID_TRACK_MAX_SLOTS, "shots: %d slots per stream (1 .. %d)", T, FID_TRACK_MAX_SLOTS);
    FID_REQUIRE(dim >= 1, "shots: dim %d must be positive", dim);
    FID_REQUIRE(finished_cap >= 1, "shots: finished_cap %d must be positive", finished_cap);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    fid_shots *sh = new fid_shots();
    sh->S = S; sh->T = T; sh->dim = dim; sh->cap = finished_cap; sh->keep_crops = keep_crops ? 1 : 0; sh->device = ctx->device;
    const size_t n = (size_t)S * T, c = (size_t)finished_cap, n_counters = 2 + 2 * (size_t)S + n;
    bool ok = hipMalloc((void **)&sh->live_meta, n * MW * 4) == hipSuccess && hipMalloc((void **)&sh->fin_meta, c * MW * 4) == hipSuccess &&
              hipMalloc((void **)&sh->live_q, n * dim * 2) == hipSuccess && hipMalloc((void **)&sh->fin_q, c * dim * 2) == hipSuccess &&
              hipMalloc((void **)&sh->counters, n_counters * 4) == hipSuccess;
    if (ok && keep_crops)
        ok = hipMalloc((void **)&sh->live_crop, n * CROP_BYTES) == hipSuccess && hipMalloc((void **)&sh->fin_crop, c * CROP_BYTES) == hipSuccess;
    if (ok) ok = ev_reserve(sh, 0) == FID_OK;
    if (!ok) {
        (void)hipGetLastError();
        free_all(sh);
        fid::set_error("shots: out of device memory for %d x %d live and %d finished records of dim %d", S, T, finished_cap, dim);
        return FID_E_NOMEM;
    }
    hipLaunchKernelGGL(shot_reset, dim3(cdiv((int)std::max(n * MW, n_counters), 256)), dim3(256), 0, ctx->stream, sh->live_meta, (int)n,
                       sh->counters, (int)n_counters);
    FID_HIP(hipGetLastError());
    *out = sh;
    return FID_OK;
}

int fid_shots_destroy(fid_ctx *ctx, fid_shots *sh) {
    FID_REQUIRE(ctx, "shots: NULL context");
    if (!sh) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    free_all(sh);
    return FID_OK;
}

int fid_track_keep(fid_ctx *ctx, fid_shots *sh, fid_tracker *trk, const int32_t *stream, int B, int cap, const int32_t *track_dev,
                   const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, int n_rows, const float *score_dev, const uint16_t *q_dev,
                   const uint8_t *crops_dev, const float *det_dev, const int32_t *ident_idx_dev, const float *ident_score_dev) {
    FID_REQUIRE(ctx && sh && trk && stream && track_dev && offsets_dev && src_dev && score_dev && q_dev && det_dev, "track keep: NULL argument");
    FID_REQUIRE(crops_dev || !sh->keep_crops, "track keep: NULL crops, the keeper was created with keep_crops");
    FID_REQUIRE((ident_idx_dev == nullptr) == (ident_score_dev == nullptr), "track keep: ident_idx and ident_score come together or not at all");
    FID_REQUIRE(sh->S == trk->S && sh->T == trk->T, "track keep: the keeper has %d x %d entries, the tracker %d x %d slots", sh->S, sh->T, trk->S,
                trk->T);
    FID_REQUIRE(B > 0 && cap > 0 && row_cap > 0, "track keep: bad sizes B %d, cap %d, row_cap %d", B, cap, row_cap);
    FID_REQUIRE(n_rows >= 0 && n_rows <= row_cap, "track keep: n_rows %d outside [0, row_cap = %d]", n_rows, row_cap);
    FID_REQUIRE(!trk->pending, "track keep: the step's fid_track_identify has not been called");
    FID_REQUIRE(trk->serial > 0, "track keep: the tracker has not run a step");
    FID_REQUIRE(B == trk->B && cap == trk->cap && row_cap == trk->row_cap && memcmp(stream, trk->stream.data(), (size_t)B * 4) == 0,
                "track keep: B, cap, row_cap or the stream array differ from the tracker's last step's");
    FID_REQUIRE(!(sh->last_trk == trk && sh->last_serial == trk->serial), "track keep: this step has been kept already");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_TRY(ev_reserve(sh, n_rows));
    sh->launches += 1;
    CopyArgs c = copy_args(sh);
    c.offsets = offsets_dev; c.q = q_dev; c.crops = crops_dev; c.n_rows = n_rows; c.B = B; c.serial = sh->launches;
    KeepArgs a{};
    a.live_meta = sh->live_meta; a.frames = sh->counters + 2; a.nfin = sh->counters + 2 + sh->S; a.live_ev = sh->counters + 2 + 2 * sh->S;
    a.ev = sh->ev; a.slots = trk->slots; a.tab = trk->tab;   // (the stream table the step stored: nobody writes it before the next step)
    a.track = track_dev; a.offsets = offsets_dev; a.src = src_dev; a.score = score_dev; a.det = det_dev;
    a.ident_idx = ident_idx_dev; a.ident_score = ident_score_dev;
    a.n_rows = n_rows; a.B = B; a.cap = cap; a.T = sh->T; a.serial = sh->launches;
    const int entries = sh->S * sh->T;
    hipLaunchKernelGGL(shot_walk, dim3(sh->S), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(shot_copy_finished, dim3(n_rows + entries), dim3(256), 0, ctx->stream, c);
    hipLaunchKernelGGL(shot_copy_live, dim3(entries), dim3(256), 0, ctx->stream, c);
    FID_HIP(hipGetLastError());
    sh->last_trk = trk;
    sh->last_serial = trk->serial;
    return FID_OK;
}

int fid_shots_flush(fid_ctx *ctx, fid_shots *sh, int stream) {
    FID_REQUIRE(ctx && sh, "shots flush: NULL argument");
    FID_REQUIRE(stream >= -1 && stream < sh->S, "shots flush: stream %d, the keeper has %d", stream, sh->S);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    sh->launches += 1;
    CopyArgs c = copy_args(sh);
    c.serial = sh->launches;                                 // (n_rows 0: slot events only, no row is read)
    const int entries = sh->S * sh->T;
    hipLaunchKernelGGL(shot_flush, dim3(sh->S), dim3(64), 0, ctx->stream, sh->live_meta, sh->counters + 2 + sh->S,
                       sh->counters + 2 + 2 * sh->S, sh->ev, sh->T, stream, sh->launches);
    hipLaunchKernelGGL(shot_copy_finished, dim3(entries), dim3(256), 0, ctx->stream, c);
    hipLaunchKernelGGL(shot_copy_live, dim3(entries), dim3(256), 0, ctx->stream, c);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_shots_finished(fid_ctx *ctx, fid_shots *sh, int32_t *count, int32_t *dropped, const int32_t **meta_dev, const uint16_t **q_dev,
                       const uint8_t **crops_dev) {
    FID_REQUIRE(ctx && sh && count && dropped, "shots finished: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    int32_t two[2] = {0, 0};
    FID_HIP(hipMemcpyAsync(two, sh->counters, 8, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    *count = two[0]; *dropped = two[1];
    if (meta_dev) *meta_dev = sh->fin_meta;
    if (q_dev) *q_dev = sh->fin_q;
    if (crops_dev) *crops_dev = sh->fin_crop;                // NULL without crops
    return FID_OK;
}

int fid_shots_clear_finished(fid_ctx *ctx, fid_shots *sh) {
    FID_REQUIRE(ctx && sh, "shots clear: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(shot_clear_finished, dim3(1), dim3(64), 0, ctx->stream, sh->counters);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_shots_read(fid_ctx *ctx, fid_shots *sh, int32_t *live_meta_host) {
    FID_REQUIRE(ctx && sh && live_meta_host, "shots read: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipMemcpyAsync(live_meta_host, sh->live_meta, (size_t)sh->S * sh->T * MW * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    return FID_OK;
}

}  // extern "C"
