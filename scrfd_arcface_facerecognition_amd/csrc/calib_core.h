// Genuine / impostor score distributions of labelled stored faces in plain loops, once, for the host twin (fid_score_hist_host, calib.hip) and
// the stand-alone sanitizer driver (tests/calib_host_driver.cpp); the bin rule and the packed keys are also what the device kernels use.
// Plain C++: no device header, no library call beyond <vector>.  The rule is include/faceid.h's (fid_gallery_score_hist);
// tests/calib_oracle.py is its executable form.
//
//   cosine = the fp32 sum of the fp16 products in ASCENDING column order, starting from +0.0f (a product of two fp16 values is exact in fp32).
//            The device sums the same products in the order of its MFMA tiles: wherever the sums are exact (the +-1 probe rows of the tests)
//            host and device are equal to the bit; elsewhere a score within summation-order rounding of a bin edge may fall on either side.
//   bin    = (int)floorf(s * (float)(bins / 2)) + bins / 2, clamped to [0, bins - 1]: ONE rounded fp32 multiply (exact for a power-of-two
//            `bins`).  The clamp is done on the float, so no out-of-range conversion to int ever happens.
//   keys   = order-preserving score bits << 32 | position word.  The score word orders every finite fp32 like the number, and -0.0 BELOW +0.0
//            (the two compare equal as numbers; a sum that starts from +0.0f never is -0.0, so this only pins the corner).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define FID_KHD __host__ __device__ inline
#else
#define FID_KHD inline
#endif

#ifndef FID_HIST_MAX_BINS
#define FID_HIST_MAX_BINS 4096            // (include/faceid.h has the same line; this header also stands alone)
#endif
#define FID_HIST_SUMMARY_WORDS 4         // positions that took part, genuine pairs, impostor pairs, non-finite pairs

FID_KHD bool fid_hist_finite(uint32_t score_bits) { return (score_bits & 0x7F800000u) != 0x7F800000u; }

// the bin of a FINITE score
FID_KHD int fid_hist_bin(float s, int bins) {
    const int half = bins / 2;
    const float f = __builtin_floorf(s * (float)half);
    return f < -(float)half ? 0 : f >= (float)half ? bins - 1 : (int)f + half;
}

// order-preserving word of a score's bits: unsigned order = the order of the numbers, -0.0 below +0.0; never 0 and never ~0 for a finite score
FID_KHD uint32_t fid_hist_sortable(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
FID_KHD uint32_t fid_hist_unsortable(uint32_t w) { return (w & 0x80000000u) ? (w & 0x7FFFFFFFu) : ~w; }
// impostor side: the MAXIMUM key is the highest score, the lowest position among equal scores; 0 = no pair
FID_KHD uint64_t fid_hist_imp_key(uint32_t score_bits, int32_t pos) { return ((uint64_t)fid_hist_sortable(score_bits) << 32) | (uint32_t)~(uint32_t)pos; }
// genuine side: the MINIMUM key is the lowest score, the lowest position among equal scores; ~0 = no pair
FID_KHD uint64_t fid_hist_gen_key(uint32_t score_bits, int32_t pos) { return ((uint64_t)fid_hist_sortable(score_bits) << 32) | (uint32_t)pos; }

inline float fid_hist_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 0x3FFu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) {
            u = sign;
        } else {                          // subnormal: man * 2^-24, exact in fp32
            float f = (float)man * 5.9604644775390625e-08f;
            memcpy(&u, &f, 4);
            u |= sign;
        }
    } else if (exp == 31) {
        u = sign | 0x7F800000u | (man << 13);
    } else {
        u = sign | ((exp + 112u) << 23) | (man << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// NULL = the arguments are fine (the host twin takes any dim >= 1; the device needs dim % 32 == 0)
inline const char *fid_score_hist_check(const void *rows_f16, int G, int dim, const int32_t *labels, int n, int bins, const uint64_t *hist,
                                        const int32_t *imp_via, const float *imp_score, const int32_t *gen_via, const float *gen_score,
                                        const uint64_t *summary) {
    if (!rows_f16 || !labels || !hist || !imp_via || !imp_score || !gen_via || !gen_score || !summary) return "NULL rows, labels or output pointer";
    if (G <= 0 || dim <= 0) return "G and dim must be positive";
    if (n <= 0) return "n must be positive";
    if (bins < 2 || bins > FID_HIST_MAX_BINS || (bins & 1)) return "bins must be even, 2 .. 4096";
    return nullptr;
}

// rows == NULL: positions = gallery rows 0 .. G - 1 (the caller passes n = G).  Outputs: hist uint64 [2][bins] (genuine, impostor), imp_via /
// gen_via int32 [n], imp_score / gen_score float [n], summary uint64 [4].
inline void fid_score_hist_table_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, int n, int bins,
                                      uint64_t *hist, int32_t *imp_via, float *imp_score, int32_t *gen_via, float *gen_score, uint64_t *summary) {
    const uint16_t *g = (const uint16_t *)rows_f16;
    std::vector<float> x((size_t)n * dim, 0.f);
    std::vector<char> part((size_t)n, 0);
    std::vector<uint64_t> ikey((size_t)n, 0ull), gkey((size_t)n, ~0ull);
    uint64_t took = 0, non_finite = 0, total[2] = {0, 0};
    for (int k = 0; k < n; k++) {
        const long long row = rows ? rows[k] : k;
        unsigned any = 0;
        if (row >= 0 && row < G)
            for (int c = 0; c < dim; c++) {
                const uint16_t h = g[(size_t)row * dim + c];
                any |= h & 0x7FFFu;
                x[(size_t)k * dim + c] = fid_hist_half(h);
            }
        part[k] = any != 0u && labels[k] >= 0;
        took += part[k];
    }
    for (size_t i = 0; i < (size_t)2 * bins; i++) hist[i] = 0;
    for (int i = 0; i < n; i++) {
        if (!part[i]) continue;
        const float *a = &x[(size_t)i * dim];
        for (int j = i + 1; j < n; j++) {
            if (!part[j]) continue;
            const float *b = &x[(size_t)j * dim];
            float s = 0.f;
            for (int c = 0; c < dim; c++) s += a[c] * b[c];
            uint32_t u;
            memcpy(&u, &s, 4);
            if (!fid_hist_finite(u)) { non_finite++; continue; }
            const int cls = labels[i] != labels[j];             // 0 genuine, 1 impostor
            hist[(size_t)cls * bins + fid_hist_bin(s, bins)]++;
            total[cls]++;
            if (cls) {
                const uint64_t ki = fid_hist_imp_key(u, j), kj = fid_hist_imp_key(u, i);
                if (ki > ikey[i]) ikey[i] = ki;
                if (kj > ikey[j]) ikey[j] = kj;
            } else {
                const uint64_t ki = fid_hist_gen_key(u, j), kj = fid_hist_gen_key(u, i);
                if (ki < gkey[i]) gkey[i] = ki;
                if (kj < gkey[j]) gkey[j] = kj;
            }
        }
    }
    for (int k = 0; k < n; k++) {
        imp_via[k] = gen_via[k] = -1;
        imp_score[k] = gen_score[k] = 0.f;
        if (ikey[k] != 0ull) {
            const uint32_t u = fid_hist_unsortable((uint32_t)(ikey[k] >> 32));
            imp_via[k] = (int32_t)~(uint32_t)ikey[k];
            memcpy(&imp_score[k], &u, 4);
        }
        if (gkey[k] != ~0ull) {
            const uint32_t u = fid_hist_unsortable((uint32_t)(gkey[k] >> 32));
            gen_via[k] = (int32_t)(uint32_t)gkey[k];
            memcpy(&gen_score[k], &u, 4);
        }
    }
    summary[0] = took; summary[1] = total[0]; summary[2] = total[1]; summary[3] = non_finite;
}
