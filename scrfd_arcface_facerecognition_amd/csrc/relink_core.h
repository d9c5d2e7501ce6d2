// The relinker's rules and its walk in plain loops, once, for the device kernel (relink.hip), the host twin (fid_track_relink_host) and the
// stand-alone sanitizer driver (tests/relink_host_driver.cpp): which detection is tracked, when a live entry begins, where a retired entry
// goes in the pool, how a row is scored against the pool and which entry it claims.  Plain inline functions, no HIP runtime call; compiles
// with a host-only compiler.  The definition is include/faceid.h's (fid_track_relink).
//
// The score is an fp32 sum of fp16 products.  A product of two fp16 values has 22 significant bits, so it is exact in fp32 with or without
// an FMA; only the order of the additions differs between the kernel and the loops here, and the contract leaves it free.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_RHD __host__ __device__ inline
#else
#define FID_RHD inline
#endif

#define FID_RELINK_MISSED_MAX 0x7FFFFFFF

FID_RHD int32_t fid_relink_raw(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_int(x);
#else
    int32_t b;
    memcpy(&b, &x, 4);
    return b;
#endif
}
FID_RHD float fid_relink_float(int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __int_as_float(b);
#else
    float x;
    memcpy(&x, &b, 4);
    return x;
#endif
}

// an fp16 value as fp32 (exact), from its bits
FID_RHD float fid_relink_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 0x3FFu;
    if (exp == 0) {                                           // zero or subnormal: man * 2^-24
        const float v = (float)man * 5.9604644775390625e-08f;
        return sign ? -v : v;
    }
    if (exp == 31) return fid_relink_float((int32_t)(sign | 0x7F800000u | (man << 13)));
    return fid_relink_float((int32_t)(sign | ((exp + 112u) << 23) | (man << 13)));
}

// is detection (id, word) tracked in one of T slots?  (-1: it touches no entry)
FID_RHD int fid_relink_slot(int32_t id, int32_t word, int T) {
    if (word < 0 || id < 0) return -1;
    const int s = word & 63;
    return s < T ? s : -1;
}

// a sighting of track `id` under `word` in a slot whose live entry holds live_id (-1: empty): does the entry begin anew?
FID_RHD bool fid_relink_begins(int32_t live_id, int32_t id, int32_t word) { return live_id != id || (word & FID_TRACK_STARTED) != 0; }

// a pool entry last seen in frame `seen` has expired in frame n  (both >= 0: the difference cannot overflow)
FID_RHD bool fid_relink_expired(int32_t n, int32_t seen, int32_t window) { return n - seen > window; }

FID_RHD bool fid_relink_config_ok(const fid_relink_config &c) {
    return c.thresh >= 0.0f && c.thresh < 1.0f && c.window >= 0 && c.max_age >= 0;            // (false for a NaN thresh)
}

inline bool fid_relink_shape_ok(int S, int T, int L, int dim) {
    return S >= 1 && (long long)S * 64 * FID_RELINK_WORDS <= 0x7FFFFFFFll && T >= 1 && T <= FID_TRACK_MAX_SLOTS && L >= 1 &&
           L <= FID_RELINK_MAX_POOL && dim >= 8 && dim % 8 == 0;
}

// argument checks shared by the device and the host entry point; NULL = fine, else what is wrong
inline const char *fid_relink_check(int S, int T, int L, int dim, const int32_t *stream, int B, int cap, const void *counts, const void *track,
                                    const void *offsets, const void *src, int row_cap, int n_rows, const void *q, const fid_relink_config *cfg,
                                    const void *person) {
    if (!stream || !counts || !track || !offsets || !src || !q || !cfg || !person) return "a NULL argument";
    if (!fid_relink_shape_ok(S, T, L, dim)) return "S < 1, T outside 1 .. 64, L outside 1 .. 64, or dim below 8 or no multiple of 8";
    if (B <= 0 || cap <= 0 || row_cap <= 0) return "B, cap or row_cap is not positive";
    if ((long long)B * cap > 0x3FFFFFFFll) return "B * cap * 2 overflows int32";
    if (n_rows < 0 || n_rows > row_cap) return "n_rows outside [0, row_cap]";
    if (!fid_relink_config_ok(*cfg)) return "a config with thresh outside [0, 1) or not finite, window < 0 or max_age < 0";
    for (int b = 0; b < B; b++)
        if (stream[b] >= S) return "a stream[b] >= S";
    return nullptr;
}

inline void fid_relink_live_clear(int32_t *w) {
    w[0] = -1;
    for (int k = 1; k < FID_RELINK_WORDS; k++) w[k] = 0;
}
inline void fid_relink_pool_clear(int32_t *w) { fid_relink_live_clear(w); }

// the fresh state (also what a reset leaves): every live entry empty, every pool entry free, q stores and frame counters zero
inline void fid_relink_state_clear(int32_t *live, uint16_t *live_q, int32_t *pool, uint16_t *pool_q, int32_t *frames, int S, int T, int L, int dim,
                                   int which) {
    for (int s = 0; s < S; s++) {
        if (which >= 0 && which != s) continue;
        for (int l = 0; l < T; l++) fid_relink_live_clear(live + ((size_t)s * T + l) * FID_RELINK_WORDS);
        for (int l = 0; l < L; l++) fid_relink_pool_clear(pool + ((size_t)s * L + l) * FID_RELINK_WORDS);
        memset(live_q + (size_t)s * T * dim, 0, (size_t)T * dim * 2);
        memset(pool_q + (size_t)s * L * dim, 0, (size_t)L * dim * 2);
        frames[s] = 0;
    }
}

// where a retiring entry goes in a stream's pool [L][8]: the lowest free index, else the smallest seen, the lowest index among equals
inline int fid_relink_pool_pick(const int32_t *pool, int L) {
    int at = -1;
    for (int p = 0; p < L; p++) {
        const int32_t *w = pool + (size_t)p * FID_RELINK_WORDS;
        if (w[0] == -1) return p;
        if (at < 0 || w[2] < pool[(size_t)at * FID_RELINK_WORDS + 2]) at = p;
    }
    return at;
}

// the live entry (words lw, embedding lq) retires into its stream's pool and becomes empty
inline void fid_relink_retire(int32_t *lw, const uint16_t *lq, int32_t *pool, uint16_t *pool_q, int L, int dim) {
    if (lw[2]) {                                              // (an entry that never had a row just vanishes)
        const int p = fid_relink_pool_pick(pool, L);
        int32_t *w = pool + (size_t)p * FID_RELINK_WORDS;
        fid_relink_pool_clear(w);
        w[0] = lw[1]; w[1] = lw[0]; w[2] = lw[4];
        memcpy(pool_q + (size_t)p * dim, lq, (size_t)dim * 2);
    }
    fid_relink_live_clear(lw);
}

// fp32 sum over dim of the fp16 products, ascending
inline float fid_relink_score(const uint16_t *a, const uint16_t *b, int dim) {
    float acc = 0.0f;
    for (int k = 0; k < dim; k++) acc += fid_relink_half(a[k]) * fid_relink_half(b[k]);
    return acc;
}

// The whole call in plain loops on host arrays (arguments already checked).  live int32 [S,T,8], live_q fp16 [S,T,dim], pool int32 [S,L,8],
// pool_q fp16 [S,L,dim], frames int32 [S]: updated in place.  Streams share nothing, so the frames are simply taken in batch order.
inline void fid_track_relink_table_host(int32_t *live, uint16_t *live_q, int32_t *pool, uint16_t *pool_q, int32_t *frames, int S, int T, int L,
                                        int dim, const int32_t *stream, int B, int cap, const int32_t *counts, const int32_t *track,
                                        const int32_t *offsets, const int32_t *src, int row_cap, int n_rows, const uint16_t *q,
                                        const fid_relink_config *cfg, int32_t *person) {
    (void)S;
    const int rows_end = n_rows < row_cap ? n_rows : row_cap;
    for (int b = 0; b < B; b++) {
        const size_t f0 = (size_t)b * cap;
        for (int f = 0; f < cap; f++) person[(f0 + f) * 2] = person[(f0 + f) * 2 + 1] = -1;
        if (stream[b] < 0) continue;
        const int s = stream[b];
        const int k = counts[b] < 0 ? 0 : (counts[b] > cap ? cap : counts[b]);
        int32_t *lv = live + (size_t)s * T * FID_RELINK_WORDS, *pl = pool + (size_t)s * L * FID_RELINK_WORDS;
        uint16_t *lq = live_q + (size_t)s * T * dim, *pq = pool_q + (size_t)s * L * dim;
        const int32_t n = frames[s];
        bool seen[FID_TRACK_MAX_SLOTS];
        for (int l = 0; l < T; l++) seen[l] = false;
        // 0. expiry
        for (int p = 0; p < L; p++) {
            int32_t *w = pl + (size_t)p * FID_RELINK_WORDS;
            if (w[0] != -1 && fid_relink_expired(n, w[2], cfg->window)) fid_relink_pool_clear(w);
        }
        // 1. sightings
        for (int f = 0; f < k; f++) {
            const int32_t t = track[(f0 + f) * 2], word = track[(f0 + f) * 2 + 1];
            const int slot = fid_relink_slot(t, word, T);
            if (slot < 0) continue;
            int32_t *w = lv + (size_t)slot * FID_RELINK_WORDS;
            if (fid_relink_begins(w[0], t, word)) {
                if (w[0] != -1) fid_relink_retire(w, lq + (size_t)slot * dim, pl, pq, L, dim);
                w[0] = w[1] = t; w[2] = w[3] = w[4] = w[5] = 0; w[6] = -1; w[7] = 0;
            }
            w[5] = 0;
            seen[slot] = true;
        }
        // 2. rows
        const int lo = offsets[b] < 0 ? 0 : offsets[b], hi = offsets[b + 1] < rows_end ? offsets[b + 1] : rows_end;
        for (int i = lo; i < hi; i++) {
            const long long face = src[i];
            if (face < (long long)f0 || face >= (long long)f0 + k) continue;
            const int slot = fid_relink_slot(track[face * 2], track[face * 2 + 1], T);
            if (slot < 0) continue;
            int32_t *w = lv + (size_t)slot * FID_RELINK_WORDS;
            const uint16_t *row = q + (size_t)i * dim;
            if (!w[2]) {
                float best = cfg->thresh;
                int at = -1;
                for (int p = 0; p < L; p++) {
                    if (pl[(size_t)p * FID_RELINK_WORDS] == -1) continue;
                    const float sc = fid_relink_score(row, pq + (size_t)p * dim, dim);
                    if (sc > best) { best = sc; at = p; }     // strict: the lowest index stays among equals; false for a NaN
                }
                if (at >= 0) {
                    int32_t *pw = pl + (size_t)at * FID_RELINK_WORDS;
                    w[1] = pw[0]; w[6] = pw[1]; w[3] = fid_relink_raw(best);
                    fid_relink_pool_clear(pw);
                }
            }
            memcpy(lq + (size_t)slot * dim, row, (size_t)dim * 2);
            w[2] = 1; w[4] = n;
        }
        // 3. output
        for (int f = 0; f < k; f++) {
            const int32_t word = track[(f0 + f) * 2 + 1];
            const int slot = fid_relink_slot(track[(f0 + f) * 2], word, T);
            if (slot < 0) continue;
            const int32_t *w = lv + (size_t)slot * FID_RELINK_WORDS;
            person[(f0 + f) * 2] = w[1];
            person[(f0 + f) * 2 + 1] = word | (w[1] != w[0] ? FID_TRACK_RELINKED : 0);
        }
        // 4. ageing
        for (int l = 0; l < T; l++) {
            int32_t *w = lv + (size_t)l * FID_RELINK_WORDS;
            if (w[0] == -1 || seen[l]) continue;
            if (w[5] < FID_RELINK_MISSED_MAX) w[5] += 1;
            if (w[5] > cfg->max_age) fid_relink_retire(w, lq + (size_t)l * dim, pl, pq, L, dim);
        }
        frames[s] = n + 1;
    }
}
