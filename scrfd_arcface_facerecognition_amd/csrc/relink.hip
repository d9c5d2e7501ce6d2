// Re-linking a returning face to its earlier track by embedding (include/faceid.h: fid_relinker_*, fid_track_relink).  The relinker follows
// the tracker: per (stream, slot) it keeps the live track's latest unit embedding, per stream a small pool of recently ended tracks, and a
// new track whose first embedding scores above a threshold against a pooled one inherits that track's person id.  (No reference analogue:
// the reference re-identifies against a gallery of names only, smart_face_recognition.py; strangers get no identity at all.)
//
// State (S x T live entries and S x L pool entries of 8 words, their fp16 rows, a frame counter per stream) lives in device memory.  One
// call is ONE launch:
//
//   relink_walk   track_walk's shape: one wave64 per stream.  Lane l owns live entry l AND pool entry l in registers (loaded once, stored
//                 once).  The stream's frames are visited in batch order; a frame's track words and its rows' face indices are loaded 64 at
//                 a time (one per lane) and handed lane to lane through v_readlane.  Everything that decides -- does an entry begin, does
//                 it retire, which pool index takes it, does a row link and to whom -- is wave-uniform: the deciding lane's words are
//                 broadcast, ballots pick indices.  Payload (a q row of dim fp16 values) moves inside the walk, as 16-byte vectors, vector
//                 v always by lane v & 63 -- in the copies live -> pool and row -> live, and in the scoring loop, which goes over the pool
//                 entries one after another, every lane multiplying its vectors of the row (vectors 0 .. 63 staged in registers once per
//                 attempt) with its vectors of the pooled row, followed by a butterfly sum.  So every address of the two q stores is
//                 only ever touched by one lane, in program order: a row that retires into the pool and is scored against two frames
//                 later in the same call needs no fence, and nothing needs LDS, a barrier or an atomic.  A link attempt is rare (a
//                 track's first row) and costs L x dim / 8 vector loads; a copy dim / 8.
//
// Frames of no stream (stream[b] < 0) get their {-1,-1} rows from workgroup b % S.  The frame-to-stream table is the one the tracker's
// last step stored (track_state.h): nobody writes it before the next step.  Nothing is read back and nothing is allocated per call.
//
// This file must never get a fast-math flag: the link score is compared bit for bit with the host twin on rows whose sums are exact.
#include "common.h"
#include "relink_core.h"
#include "track_state.h"

struct fid_relinker {
    int S = 0, T = 0, L = 0, dim = 0, device = 0;
    int32_t *live = nullptr, *pool = nullptr, *frames = nullptr;      // [S*T][8], [S*L][8], [S]
    uint16_t *live_q = nullptr, *pool_q = nullptr;                    // [S*T][dim], [S*L][dim]
    const fid_tracker *last_trk = nullptr;                            // the step the last relink followed
    unsigned long long last_serial = 0;
};

namespace {

using fid::cdiv;

constexpr int RW = FID_RELINK_WORDS;
static_assert(RW == 8, "entries are moved as two 16-byte vectors");

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(lane_i(__float_as_int(v), l)); }

__device__ __forceinline__ float h2f(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
__device__ __forceinline__ float dot2(uint32_t x, uint32_t y, float acc) {
    acc = fmaf(h2f(x & 0xFFFFu), h2f(y & 0xFFFFu), acc);     // (the product is exact in fp32: the FMA rounds what mul + add round)
    return fmaf(h2f(x >> 16), h2f(y >> 16), acc);
}
__device__ __forceinline__ float dot8(const uint4 x, const uint4 y, float acc) {
    return dot2(x.w, y.w, dot2(x.z, y.z, dot2(x.y, y.y, dot2(x.x, y.x, acc))));
}

// vector v of a caller's row: 16 bytes at once where the pointer allows it
__device__ __forceinline__ uint4 row_vec(const uint16_t *row, int v, bool aligned) {
    if (aligned) return ((const uint4 *)row)[v];
    const uint16_t *p = row + (size_t)v * 8;
    return make_uint4((uint32_t)p[0] | ((uint32_t)p[1] << 16), (uint32_t)p[2] | ((uint32_t)p[3] << 16), (uint32_t)p[4] | ((uint32_t)p[5] << 16),
                      (uint32_t)p[6] | ((uint32_t)p[7] << 16));
}

struct WalkArgs {
    int32_t *live, *pool, *frames;
    uint16_t *live_q, *pool_q;
    const int32_t *tab;                                      // [B] stream of frame b (the tracker's)
    const int32_t *counts, *track, *offsets, *src;
    const uint16_t *q;
    int32_t *person;
    fid_relink_config cfg;
    int n_rows, B, cap, S, T, L, dim;                        // n_rows: already min(n_rows, row_cap)
};

__global__ void __launch_bounds__(64) relink_walk(const WalkArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool mine = lane < a.T, pmine = lane < a.L;
    const int nv = a.dim / 8;
    const bool q_aligned = ((uintptr_t)a.q & 15u) == 0u;
    int32_t *lw = a.live + ((size_t)s * a.T + (mine ? lane : 0)) * RW;
    int32_t *pw = a.pool + ((size_t)s * a.L + (pmine ? lane : 0)) * RW;
    uint16_t *live_q = a.live_q + (size_t)s * a.T * a.dim, *pool_q = a.pool_q + (size_t)s * a.L * a.dim;
    int id = -1, person = 0, has_q = 0, sbits = 0, seen = 0, missed = 0, from = 0;            // live entry `lane`
    int p_person = -1, p_id = 0, p_seen = 0;                                                  // pool entry `lane`
    if (mine) {
        const int4 x = ((const int4 *)lw)[0], y = ((const int4 *)lw)[1];
        id = x.x; person = x.y; has_q = x.z; sbits = x.w; seen = y.x; missed = y.y; from = y.z;
    }
    if (pmine) {
        const int4 x = ((const int4 *)pw)[0];
        p_person = x.x; p_id = x.y; p_seen = x.z;
    }
    int n = a.frames[s];                                     // (the same in every lane)

    // live entry `slot` (wave-uniform; it has a row) goes into the pool: the lowest free index, else the smallest seen, the lowest index
    auto retire = [&](int slot) {
        const int r_person = lane_i(person, slot), r_id = lane_i(id, slot), r_seen = lane_i(seen, slot);
        const unsigned long long fr = __ballot(pmine && p_person == -1);
        int p;
        if (fr != 0ull) {
            p = __ffsll((long long)fr) - 1;
        } else {
            unsigned long long key = pmine ? (((unsigned long long)(uint32_t)p_seen << 8) | (unsigned)lane) : ~0ull;     // (seen >= 0)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(key, o);
                key = other < key ? other : key;
            }
            p = (int)(key & 255ull);
        }
        p = __builtin_amdgcn_readfirstlane(p);
        const uint4 *from_q = (const uint4 *)(live_q + (size_t)slot * a.dim);
        uint4 *to_q = (uint4 *)(pool_q + (size_t)p * a.dim);
        for (int v = lane; v < nv; v += 64) to_q[v] = from_q[v];
        if (lane == p) { p_person = r_person; p_id = r_id; p_seen = r_seen; }
    };

    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int nb = min(64, a.B - b0);
        int f_stream = -1, f_k = 0, f_lo = 0, f_hi = 0;
        if (lane < nb) {
            f_stream = a.tab[b0 + lane];
            f_k = min(max(a.counts[b0 + lane], 0), a.cap);
            f_lo = a.offsets[b0 + lane]; f_hi = a.offsets[b0 + lane + 1];
        }
        for (int jb = 0; jb < nb; jb++) {
            const int b = b0 + jb, fs = lane_i(f_stream, jb);
            const size_t face0 = (size_t)b * a.cap;
            if (fs != s) {                                   // (wave-uniform)
                if (fs < 0 && b % a.S == s)                  // a frame of no stream: its rows are written once, by this workgroup
                    for (int f = lane; f < a.cap; f += 64) *(int2 *)(a.person + (face0 + f) * 2) = make_int2(-1, -1);
                continue;
            }
            const int k = lane_i(f_k, jb);
            // 0. expiry
            if (pmine && p_person != -1 && fid_relink_expired(n, p_seen, a.cfg.window)) { p_person = -1; p_id = 0; p_seen = 0; }
            // 1. sightings
            unsigned long long seen_mask = 0ull;             // (wave-uniform)
            for (int f0 = 0; f0 < k; f0 += 64) {
                int tid = -1, word = -1;
                if (f0 + lane < k) {
                    const int2 t = *(const int2 *)(a.track + (face0 + f0 + lane) * 2);
                    tid = t.x; word = t.y;
                }
                const int slotv = fid_relink_slot(tid, word, a.T);
                unsigned long long work = __ballot(slotv >= 0);
                while (work != 0ull) {                       // (wave-uniform) in detection order
                    const int j = __ffsll((long long)work) - 1;
                    work &= work - 1ull;
                    const int slot = lane_i(slotv, j), t = lane_i(tid, j), w = lane_i(word, j);
                    const bool begins = lane == slot && fid_relink_begins(id, t, w);
                    if (__ballot(begins) != 0ull) {
                        if (__ballot(begins && id != -1 && has_q != 0) != 0ull) retire(slot);
                        if (lane == slot) { id = t; person = t; has_q = 0; sbits = 0; seen = 0; missed = 0; from = -1; }
                    }
                    if (lane == slot) missed = 0;
                    seen_mask |= 1ull << slot;
                }
            }
            // 2. rows
            const int r1 = min(lane_i(f_hi, jb), a.n_rows);
            for (int i0 = max(lane_i(f_lo, jb), 0); i0 < r1; i0 += 64) {
                int tid = -1, word = -1;
                if (i0 + lane < r1) {
                    const long long face = a.src[i0 + lane];
                    if (face >= (long long)face0 && face < (long long)face0 + k) {
                        const int2 t = *(const int2 *)(a.track + (size_t)face * 2);
                        tid = t.x; word = t.y;
                    }
                }
                const int slotv = fid_relink_slot(tid, word, a.T);
                unsigned long long work = __ballot(slotv >= 0);
                while (work != 0ull) {                       // (wave-uniform) in table order
                    const int j = __ffsll((long long)work) - 1;
                    work &= work - 1ull;
                    const int slot = lane_i(slotv, j);
                    const uint16_t *row = a.q + (size_t)(i0 + j) * a.dim;
                    unsigned long long cand = lane_i(has_q, slot) == 0 ? __ballot(pmine && p_person != -1) : 0ull;
                    if (cand != 0ull) {                      // the track's first row: a link attempt
                        uint4 r0 = make_uint4(0u, 0u, 0u, 0u);
                        if (lane < nv) r0 = row_vec(row, lane, q_aligned);       // the row, staged once
                        float best = a.cfg.thresh;
                        int at = -1;
                        while (cand != 0ull) {               // ascending pool index: the lowest stays among equals
                            const int p = __ffsll((long long)cand) - 1;
                            cand &= cand - 1ull;
                            const uint4 *pq = (const uint4 *)(pool_q + (size_t)p * a.dim);
                            float acc = 0.0f;
                            if (lane < nv) acc = dot8(r0, pq[lane], acc);
                            for (int v = lane + 64; v < nv; v += 64) acc = dot8(row_vec(row, v, q_aligned), pq[v], acc);
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                            acc = lane_f(acc, 0);
                            if (acc > best) { best = acc; at = p; }              // strict; false for a NaN
                        }
                        if (at >= 0) {
                            const int r_person = lane_i(p_person, at), r_id = lane_i(p_id, at);
                            if (lane == slot) { person = r_person; from = r_id; sbits = __float_as_int(best); }
                            if (lane == at) { p_person = -1; p_id = 0; p_seen = 0; }             // a pooled track is claimed once
                        }
                    }
                    uint4 *to_q = (uint4 *)(live_q + (size_t)slot * a.dim);
                    for (int v = lane; v < nv; v += 64) to_q[v] = row_vec(row, v, q_aligned);
                    if (lane == slot) { has_q = 1; seen = n; }
                }
            }
            // 3. output
            for (int f0 = 0; f0 < a.cap; f0 += 64) {
                const int f = f0 + lane;
                int tid = -1, word = -1;
                if (f < k) {
                    const int2 t = *(const int2 *)(a.track + (face0 + f) * 2);
                    tid = t.x; word = t.y;
                }
                const int slot = fid_relink_slot(tid, word, a.T);
                const int l_person = __shfl(person, max(slot, 0)), l_id = __shfl(id, max(slot, 0));
                if (f < a.cap)
                    *(int2 *)(a.person + (face0 + f) * 2) =
                        slot >= 0 ? make_int2(l_person, word | (l_person != l_id ? FID_TRACK_RELINKED : 0)) : make_int2(-1, -1);
            }
            // 4. ageing, slots ascending
            const bool unseen = mine && id != -1 && ((seen_mask >> lane) & 1ull) == 0ull;
            if (unseen && missed < FID_RELINK_MISSED_MAX) missed += 1;
            const bool ends = unseen && missed > a.cfg.max_age;
            unsigned long long gone = __ballot(ends && has_q != 0);
            while (gone != 0ull) {                           // (wave-uniform)
                const int slot = __ffsll((long long)gone) - 1;
                gone &= gone - 1ull;
                retire(slot);
            }
            if (ends) { id = -1; person = has_q = sbits = seen = missed = from = 0; }
            n += 1;
        }
    }
    if (mine) {
        ((int4 *)lw)[0] = make_int4(id, person, has_q, sbits);
        ((int4 *)lw)[1] = make_int4(seen, missed, from, 0);
    }
    if (pmine) {
        ((int4 *)pw)[0] = make_int4(p_person, p_id, p_seen, 0);
        ((int4 *)pw)[1] = make_int4(0, 0, 0, 0);
    }
    if (lane == 0) a.frames[s] = n;
}

// workgroup s: stream s.  `which` (-1: every stream) gets the fresh state: empty live entries, a free pool, zero rows, frame 0
__global__ void __launch_bounds__(256) relink_reset(int32_t *live, int32_t *pool, int32_t *frames, uint16_t *live_q, uint16_t *pool_q, int T, int L,
                                                    int dim, int which) {
    const int s = blockIdx.x, t = threadIdx.x;
    if (which >= 0 && which != s) return;
    for (int i = t; i < T * RW; i += 256) live[(size_t)s * T * RW + i] = i % RW == 0 ? -1 : 0;
    for (int i = t; i < L * RW; i += 256) pool[(size_t)s * L * RW + i] = i % RW == 0 ? -1 : 0;
    uint4 *lq = (uint4 *)(live_q + (size_t)s * T * dim), *pq = (uint4 *)(pool_q + (size_t)s * L * dim);
    for (int i = t; i < T * (dim / 8); i += 256) lq[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = t; i < L * (dim / 8); i += 256) pq[i] = make_uint4(0u, 0u, 0u, 0u);
    if (t == 0) frames[s] = 0;
}

void free_all(fid_relinker *r) {
    for (void *p : {(void *)r->live, (void *)r->pool, (void *)r->frames, (void *)r->live_q, (void *)r->pool_q})
        if (p) (void)hipFree(p);
    delete r;
}

void launch_reset(fid_ctx *ctx, fid_relinker *r, int which) {
    hipLaunchKernelGGL(relink_reset, dim3(r->S), dim3(256), 0, ctx->stream, r->live, r->pool, r->frames, r->live_q, r->pool_q, r->T, r->L, r->dim,
                       which);
}

}  // namespace

extern "C" {

int fid_relinker_create(fid_ctx *ctx, int S, int T, int L, int dim, fid_relinker **out) {
    FID_REQUIRE(ctx && out, "relinker: NULL argument");
    FID_REQUIRE(fid_relink_shape_ok(S, T, L, dim),
                "relinker: %d streams x %d slots (1 .. %d), a pool of %d (1 .. %d), dim %d (>= 8, a multiple of 8)", S, T, FID_TRACK_MAX_SLOTS, L,
                FID_RELINK_MAX_POOL, dim);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    fid_relinker *r = new fid_relinker();
    r->S = S; r->T = T; r->L = L; r->dim = dim; r->device = ctx->device;
    const size_t nl = (size_t)S * T, np = (size_t)S * L;
    const bool ok = hipMalloc((void **)&r->live, nl * RW * 4) == hipSuccess && hipMalloc((void **)&r->pool, np * RW * 4) == hipSuccess &&
                    hipMalloc((void **)&r->frames, (size_t)S * 4) == hipSuccess && hipMalloc((void **)&r->live_q, nl * dim * 2) == hipSuccess &&
                    hipMalloc((void **)&r->pool_q, np * dim * 2) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        free_all(r);
        fid::set_error("relinker: out of device memory for %d x (%d + %d) entries of dim %d", S, T, L, dim);
        return FID_E_NOMEM;
    }
    launch_reset(ctx, r, -1);
    FID_HIP(hipGetLastError());
    *out = r;
    return FID_OK;
}

int fid_relinker_destroy(fid_ctx *ctx, fid_relinker *r) {
    FID_REQUIRE(ctx, "relinker: NULL context");
    if (!r) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    free_all(r);
    return FID_OK;
}

int fid_relinker_reset(fid_ctx *ctx, fid_relinker *r, int stream) {
    FID_REQUIRE(ctx && r, "relinker reset: NULL argument");
    FID_REQUIRE(stream >= -1 && stream < r->S, "relinker reset: stream %d, the relinker has %d", stream, r->S);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    launch_reset(ctx, r, stream);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_relinker_read(fid_ctx *ctx, fid_relinker *r, int32_t *live_host, int32_t *pool_host, int32_t *frames_host, uint16_t *live_q_host,
                      uint16_t *pool_q_host) {
    FID_REQUIRE(ctx && r && live_host && pool_host && frames_host, "relinker read: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    const size_t nl = (size_t)r->S * r->T, np = (size_t)r->S * r->L;
    FID_HIP(hipMemcpyAsync(live_host, r->live, nl * RW * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipMemcpyAsync(pool_host, r->pool, np * RW * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipMemcpyAsync(frames_host, r->frames, (size_t)r->S * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (live_q_host) FID_HIP(hipMemcpyAsync(live_q_host, r->live_q, nl * r->dim * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (pool_q_host) FID_HIP(hipMemcpyAsync(pool_q_host, r->pool_q, np * r->dim * 2, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    return FID_OK;
}

int fid_track_relink(fid_ctx *ctx, fid_relinker *r, fid_tracker *trk, const int32_t *stream, int B, int cap, const int32_t *counts_dev,
                     const int32_t *track_dev, const int32_t *offsets_dev, const int32_t *src_dev, int row_cap, int n_rows, const uint16_t *q_dev,
                     const fid_relink_config *cfg, int32_t *person_dev) {
    FID_REQUIRE(ctx && r && trk, "track relink: NULL argument");
    const char *why = fid_relink_check(r->S, r->T, r->L, r->dim, stream, B, cap, counts_dev, track_dev, offsets_dev, src_dev, row_cap, n_rows,
                                       q_dev, cfg, person_dev);
    FID_REQUIRE(why == nullptr, "track relink: %s", why ? why : "");
    FID_REQUIRE(r->S == trk->S && r->T == trk->T, "track relink: the relinker has %d x %d entries, the tracker %d x %d slots", r->S, r->T, trk->S,
                trk->T);
    FID_REQUIRE(!trk->pending, "track relink: the step's fid_track_identify has not been called");
    FID_REQUIRE(trk->serial > 0, "track relink: the tracker has not run a step");
    FID_REQUIRE(B == trk->B && cap == trk->cap && row_cap == trk->row_cap && memcmp(stream, trk->stream.data(), (size_t)B * 4) == 0,
                "track relink: B, cap, row_cap or the stream array differ from the tracker's last step's");
    FID_REQUIRE(!(r->last_trk == trk && r->last_serial == trk->serial), "track relink: this step has been relinked already");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    WalkArgs a{};
    a.live = r->live; a.pool = r->pool; a.frames = r->frames; a.live_q = r->live_q; a.pool_q = r->pool_q;
    a.tab = trk->tab;                                        // (the stream table the step stored: nobody writes it before the next step)
    a.counts = counts_dev; a.track = track_dev; a.offsets = offsets_dev; a.src = src_dev; a.q = q_dev; a.person = person_dev;
    a.cfg = *cfg; a.n_rows = n_rows; a.B = B; a.cap = cap; a.S = r->S; a.T = r->T; a.L = r->L; a.dim = r->dim;
    hipLaunchKernelGGL(relink_walk, dim3(r->S), dim3(64), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    r->last_trk = trk;
    r->last_serial = trk->serial;
    return FID_OK;
}

int fid_track_relink_host(int32_t *live, uint16_t *live_q, int32_t *pool, uint16_t *pool_q, int32_t *frames, int S, int T, int L, int dim,
                          const int32_t *stream, int B, int cap, const int32_t *counts, const int32_t *track, const int32_t *offsets,
                          const int32_t *src, int row_cap, int n_rows, const uint16_t *q, const fid_relink_config *cfg, int32_t *person) {
    FID_REQUIRE(live && live_q && pool && pool_q && frames, "track relink: NULL state");
    const char *why = fid_relink_check(S, T, L, dim, stream, B, cap, counts, track, offsets, src, row_cap, n_rows, q, cfg, person);
    FID_REQUIRE(why == nullptr, "track relink: %s", why ? why : "");
    fid_track_relink_table_host(live, live_q, pool, pool_q, frames, S, T, L, dim, stream, B, cap, counts, track, offsets, src, row_cap, n_rows, q,
                                cfg, person);
    return FID_OK;
}

}  // extern "C"
