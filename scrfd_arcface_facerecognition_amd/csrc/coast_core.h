// The coaster's arithmetic and its walk in plain loops, once, for the device kernels (coast.hip), the host twin (fid_track_coast_host) and the
// stand-alone sanitizer driver (tests/coast_host_driver.cpp): how one entry takes a detection, how it ages at the end of a frame, and the box
// it emits while it coasts.  Plain inline functions, no HIP runtime call; compiles with a host-only compiler.  The definition is
// include/faceid.h's (fid_track_coast).
//
// Every translation unit that includes this must be built with -ffp-contract=off and without any fast-math flag: every operation is
// rounded on its own (the multiply of a prediction before its add: no FMA) and the divide is the correctly rounded one.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_CHD __host__ __device__ inline
#else
#define FID_CHD inline
#endif

#define FID_COAST_MISSED_MAX (1 << 20)
#define FID_COAST_QNAN 0x7FC00000

FID_CHD float fid_coast_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
FID_CHD int32_t fid_coast_raw(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_int(x);
#else
    int32_t b;
    memcpy(&b, &x, 4);
    return b;
#endif
}
FID_CHD float fid_coast_float(int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __int_as_float(b);
#else
    float x;
    memcpy(&x, &b, 4);
    return x;
#endif
}
// the bits a float is stored with: a NaN leaves as THE quiet NaN (IEEE 754 fixes neither sign nor payload, and hosts and devices differ)
FID_CHD int32_t fid_coast_bits(float x) { return x == x ? fid_coast_raw(x) : (int32_t)FID_COAST_QNAN; }
FID_CHD float fid_coast_canon(float x) { return fid_coast_float(fid_coast_bits(x)); }

// one entry, as the walk holds it (the state's words 0 .. 13; 14 and 15 are 0)
struct fid_coast_entry {
    int32_t id, missed, has_vel, ident_idx, ident_score;     // ident_score: the float's bits
    float box[4], vel[4], conf;
};

FID_CHD void fid_coast_entry_clear(fid_coast_entry &e) {
    e.id = -1; e.missed = e.has_vel = e.ident_idx = e.ident_score = 0;
    for (int k = 0; k < 4; k++) e.box[k] = e.vel[k] = 0.0f;
    e.conf = 0.0f;
}
FID_CHD void fid_coast_entry_load(fid_coast_entry &e, const int32_t *w) {
    e.id = w[0]; e.missed = w[1]; e.has_vel = w[2]; e.ident_idx = w[3]; e.ident_score = w[4];
    for (int k = 0; k < 4; k++) { e.box[k] = fid_coast_float(w[5 + k]); e.vel[k] = fid_coast_float(w[9 + k]); }
    e.conf = fid_coast_float(w[13]);
}
FID_CHD void fid_coast_entry_store(const fid_coast_entry &e, int32_t *w) {
    w[0] = e.id; w[1] = e.missed; w[2] = e.has_vel; w[3] = e.ident_idx; w[4] = e.ident_score;
    for (int k = 0; k < 4; k++) { w[5 + k] = fid_coast_bits(e.box[k]); w[9 + k] = fid_coast_bits(e.vel[k]); }
    w[13] = fid_coast_bits(e.conf);
    w[14] = w[15] = 0;
}

// is detection (id, word) tracked in one of T slots?  (-1: it touches no entry)
FID_CHD int fid_coast_slot(int32_t id, int32_t word, int T) {
    if (word < 0 || id < 0) return -1;
    const int s = word & 0xFF;
    return s < T ? s : -1;
}

// the entry takes the frame's detection of its slot: det[5], the identity (ident_score as bits)
FID_CHD void fid_coast_take(fid_coast_entry &e, int32_t id, int32_t word, const float *det, int32_t ident_idx, int32_t ident_score) {
    if (e.id == id && !(word & FID_TRACK_STARTED)) {          // the track continues: the velocity over the gap
        const float d = (float)(e.missed + 1);
        for (int k = 0; k < 4; k++) e.vel[k] = fid_coast_canon(fid_coast_div(det[k] - e.box[k], d));
        e.has_vel = 1;
    } else {
        e.id = id;
        for (int k = 0; k < 4; k++) e.vel[k] = 0.0f;
        e.has_vel = 0;
    }
    for (int k = 0; k < 4; k++) e.box[k] = fid_coast_canon(det[k]);
    e.conf = fid_coast_canon(det[4]);
    e.missed = 0;
    e.ident_idx = ident_idx;
    e.ident_score = fid_coast_bits(fid_coast_float(ident_score));
}

// the end of a frame in which the (live) entry was not matched: it ages, and says whether it coasts in this frame and where
FID_CHD bool fid_coast_age(fid_coast_entry &e, const fid_coast_config &c, float *out) {
    e.missed = e.missed + 1 < FID_COAST_MISSED_MAX ? e.missed + 1 : FID_COAST_MISSED_MAX;
    if (e.missed > c.hold) return false;                      // (missed >= 1 here)
    const float m = (float)e.missed;
    float p[4];
    for (int k = 0; k < 4; k++) {
        p[k] = e.box[k];
        if (c.predict && e.has_vel) {
            const float step = e.vel[k] * m;                  // rounded, then added
            p[k] = e.box[k] + step;
        }
    }
    if (c.grow != 0.0f) {                                     // grow = 0 skips the step: the box leaves bit for bit, -0.0 and inf included
        const float g = c.grow * m;
        const float dx = g * (p[2] - p[0]), dy = g * (p[3] - p[1]);
        const float x1 = p[0] - dx, y1 = p[1] - dy, x2 = p[2] + dx, y2 = p[3] + dy;
        p[0] = x1; p[1] = y1; p[2] = x2; p[3] = y2;
    }
    for (int k = 0; k < 4; k++) out[k] = fid_coast_canon(p[k]);
    return true;
}

FID_CHD bool fid_coast_config_ok(const fid_coast_config &c) {
    return c.hold >= 0 && c.hold <= 1023 && c.grow >= 0.0f && c.grow <= 0.5f && c.reserved == 0;      // (false for a NaN grow)
}

// argument checks shared by the device and the host entry point; NULL = fine, else what is wrong
inline const char *fid_coast_check(int S, int T, const int32_t *stream, int B, int cap, const void *det, const void *counts, const void *track,
                                   const void *ident_idx, const void *ident_score, const fid_coast_config *cfg, const void *det_out,
                                   const void *counts_out, const void *track_out, const void *idx_out, const void *score_out) {
    if (!stream || !det || !counts || !track || !cfg || !det_out || !counts_out || !track_out || !idx_out || !score_out) return "a NULL argument";
    if ((ident_idx == nullptr) != (ident_score == nullptr)) return "ident_idx and ident_score come together or not at all";
    if (S < 1 || T < 1 || T > FID_TRACK_MAX_SLOTS) return "S < 1 or T outside 1 .. 64";
    if (B <= 0 || cap <= 0) return "B or cap is not positive";
    if ((long long)B * ((long long)cap + T) > 0x7FFFFFFFll) return "B * (cap + T) overflows int32";
    if (!fid_coast_config_ok(*cfg)) return "a config with hold outside [0, 1023], grow outside [0, 0.5] or NaN, or reserved != 0";
    for (int b = 0; b < B; b++)
        if (stream[b] >= S) return "a stream[b] >= S";
    return nullptr;
}

// output row i of frame b is empty
inline void fid_coast_filler(size_t at, float *det_out, int32_t *track_out, int32_t *idx_out, float *score_out) {
    for (int k = 0; k < 5; k++) det_out[at * 5 + k] = 0.0f;
    track_out[at * 2] = track_out[at * 2 + 1] = -1;
    idx_out[at] = -1;
    score_out[at] = 0.0f;
}

// The whole call in plain loops on host arrays (arguments already checked).  entries: int32 [S,T,FID_COAST_WORDS], updated in place.
inline void fid_track_coast_table_host(int32_t *entries, int S, int T, const int32_t *stream, int B, int cap, const float *det,
                                       const int32_t *counts, const int32_t *track, const int32_t *ident_idx, const float *ident_score,
                                       const fid_coast_config *cfg, float *det_out, int32_t *counts_out, int32_t *track_out, int32_t *idx_out,
                                       float *score_out) {
    const int cap2 = cap + T;
    (void)S;
    for (int b = 0; b < B; b++) {
        const size_t in0 = (size_t)b * cap, out0 = (size_t)b * cap2;
        int n = 0;
        if (stream[b] >= 0) {
            const int s = stream[b];
            const int k = counts[b] < 0 ? 0 : (counts[b] > cap ? cap : counts[b]);
            int pick[FID_TRACK_MAX_SLOTS];                    // per slot the HIGHEST detection that names it
            for (int l = 0; l < T; l++) pick[l] = -1;
            for (int f = 0; f < k; f++) {
                const int slot = fid_coast_slot(track[(in0 + f) * 2], track[(in0 + f) * 2 + 1], T);
                if (slot >= 0) pick[slot] = f;
                memcpy(det_out + (out0 + f) * 5, det + (in0 + f) * 5, 20);
                track_out[(out0 + f) * 2] = track[(in0 + f) * 2];
                track_out[(out0 + f) * 2 + 1] = track[(in0 + f) * 2 + 1];
                idx_out[out0 + f] = ident_idx ? ident_idx[in0 + f] : -1;
                if (ident_score) memcpy(score_out + out0 + f, ident_score + in0 + f, 4);
                else score_out[out0 + f] = 0.0f;
            }
            n = k;
            for (int l = 0; l < T; l++) {
                int32_t *w = entries + ((size_t)s * T + l) * FID_COAST_WORDS;
                fid_coast_entry e;
                fid_coast_entry_load(e, w);
                float box[4];
                if (pick[l] >= 0) {
                    const size_t f = in0 + pick[l];
                    int32_t is = 0;
                    if (ident_score) memcpy(&is, ident_score + f, 4);
                    fid_coast_take(e, track[f * 2], track[f * 2 + 1], det + f * 5, ident_idx ? ident_idx[f] : -1, is);
                } else if (e.id >= 0 && fid_coast_age(e, *cfg, box)) {
                    const size_t at = out0 + n;
                    for (int q = 0; q < 4; q++) { const int32_t v = fid_coast_bits(box[q]); memcpy(det_out + at * 5 + q, &v, 4); }
                    const int32_t cb = fid_coast_bits(e.conf);
                    memcpy(det_out + at * 5 + 4, &cb, 4);
                    track_out[at * 2] = e.id;
                    track_out[at * 2 + 1] = l | FID_TRACK_COASTED | (e.missed << 16);
                    idx_out[at] = e.ident_idx;
                    memcpy(score_out + at, &e.ident_score, 4);
                    n += 1;
                }
                fid_coast_entry_store(e, w);
            }
        }
        counts_out[b] = n;
        for (int i = n; i < cap2; i++) fid_coast_filler(out0 + i, det_out, track_out, idx_out, score_out);
    }
}
