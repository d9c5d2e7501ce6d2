// Identity templates -- one gallery row per person from many stored faces -- the arithmetic once, for the device kernels (template.hip), the
// host twin (fid_templates_host) and the stand-alone sanitizer driver (tests/template_host_driver.cpp).  Plain C++: no device header, no
// library call beyond <vector>.  The rule is include/faceid.h's (fid_gallery_templates); tests/template_oracle.py is its executable form.
//
//   fixed    an fp16 element with |x| <= 2 is an integer multiple of 2^-24: X = x * 2^24 is an exact int32 with |X| <= 2^25.
//   sum      S_pc = sum of w_k * X_kc over the members of person p in int64: |S| <= 2^20 * 255 * 2^25 < 2^53, so neither the sum nor its
//            conversion to double rounds, and the order of the additions cannot matter.
//   norm     the ONE floating-point reduction, so its order is pinned: q_c = (double)S_c * (double)S_c; lane l of 64 owns the columns c with
//            (c / 8) % 64 == l (eight consecutive columns of every block of 512: what a 16-byte load per lane of a wave brings) and adds its
//            q_c in ascending c, starting from +0.0; six butterfly rounds with XOR partners 32, 16, 8, 4, 2, 1; sqrt.  Every operation is a
//            separately rounded IEEE fp64 operation (build with -ffp-contract=off).
//   template t_c = (double)S_c / nrm, rounded to fp32, then to fp16 (both to nearest even; fid_tpl_f32_to_f16 is the second rounding in integer
//            arithmetic, the same on every machine).  nrm == 0: the all-zero row.
//   score    D_k = sum of X_kc * T_c in int64 (T = the fp16 template as an integer; |D| <= 2^49 * dim), score = (float)((double)D * 2^-48).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define FID_THD __host__ __device__ inline
#else
#define FID_THD inline
#endif

#ifndef FID_TEMPLATE_MAX_ROWS
#define FID_TEMPLATE_MAX_ROWS (1 << 20)   // (include/faceid.h has the same lines; this header also stands alone)
#define FID_TEMPLATE_MAX_DIM 4096
#define FID_TEMPLATE_CHUNK 256
#endif
#define FID_TEMPLATE_SUMMARY_WORDS 6      // took part, persons with a member, persons with a zero template, dropped, rejected for their elements, 0

// finite and |x| <= 2 (the bits of 2.0 are 0x4000; every inf and NaN lies above)
FID_THD bool fid_tpl_elem_ok(uint16_t h) { return (h & 0x7FFFu) <= 0x4000u; }

// x * 2^24 of an element that passed fid_tpl_elem_ok (exponent field <= 16, so the shift stays below 2^26)
FID_THD int32_t fid_tpl_fixed(uint16_t h) {
    const int32_t e = (h >> 10) & 31, m = h & 0x3FF;
    const int32_t mag = e == 0 ? m : (int32_t)((uint32_t)(1024 + m) << (e - 1));
    return (h & 0x8000u) ? -mag : mag;
}

// fp32 -> fp16 bits, round to nearest even, subnormal results kept (what numpy's astype(float16) and v_cvt_f16_f32 do)
FID_THD uint16_t fid_tpl_f32_to_f16(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7FFFFFFFu;
    if (u >= 0x47800000u) return (uint16_t)(sign | (u > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (u < 0x38800000u) {                          // below 2^-14: a subnormal half = the value in units of 2^-24, rounded
        if (u < 0x33000000u) return (uint16_t)sign; // below 2^-25
        const int shift = 126 - (int)(u >> 23);     // 14 .. 24
        const uint32_t man = (u & 0x7FFFFFu) | 0x800000u;
        const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        return (uint16_t)(sign | (q + (rem > half || (rem == half && (q & 1u)))));
    }
    const uint32_t man = u & 0x7FFFFFu, rem = man & 0x1FFFu;
    uint32_t r = (((u >> 23) - 112u) << 10) | (man >> 13);
    r += (rem > 0x1000u || (rem == 0x1000u && (r & 1u)));      // (a carry runs into the exponent, up to infinity, as it should)
    return (uint16_t)(sign | r);
}

// order-preserving word of a score's bits: unsigned order = the order of the numbers (-0.0 below +0.0; a score here never is -0.0)
FID_THD uint32_t fid_tpl_sortable(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
// lowest score, lowest position among equals: the MINIMUM of this key; ~0 = no member
FID_THD uint64_t fid_tpl_low_key(uint32_t score_bits, int32_t pos) { return ((uint64_t)fid_tpl_sortable(score_bits) << 32) | (uint32_t)pos; }
// highest score, lowest position among equals: the MAXIMUM of this key; 0 = no member
FID_THD uint64_t fid_tpl_high_key(uint32_t score_bits, int32_t pos) { return ((uint64_t)fid_tpl_sortable(score_bits) << 32) | (uint32_t)~(uint32_t)pos; }

FID_THD float fid_tpl_score(int64_t D) { return (float)((double)D * 0x1p-48); }
FID_THD bool fid_tpl_keeps(float score, float min_score) { return min_score <= -2.0f || score >= min_score; }
FID_THD float fid_tpl_element(int64_t S, double nrm) { return (float)((double)S / nrm); }
FID_THD float fid_tpl_cohesion(double nrm, int64_t W) { return nrm > 0.0 ? (float)(nrm / ((double)W * 16777216.0)) : 0.f; }

// the pinned norm of S[0 .. dim)
inline double fid_tpl_norm_host(const int64_t *S, int dim) {
    double lane[64], next[64];
    for (int l = 0; l < 64; l++) lane[l] = 0.0;
    for (int c = 0; c < dim; c++) {                 // ascending c: every lane receives its columns in ascending order
        const double d = (double)S[c];
        const double q = d * d;
        lane[(c >> 3) & 63] = lane[(c >> 3) & 63] + q;
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; l++) next[l] = lane[l] + lane[l ^ o];
        for (int l = 0; l < 64; l++) lane[l] = next[l];
    }
    return __builtin_sqrt(lane[0]);
}

// NULL = the arguments are fine (the host twin takes any dim 1 .. 4096; the device needs dim % 32 == 0)
inline const char *fid_templates_check(const void *rows_f16, long long G, int dim, const int32_t *labels, int n, int P, float min_score,
                                       const void *templates, const float *score, const int32_t *kept, const int32_t *person,
                                       const float *cohesion, const int64_t *summary) {
    if (!rows_f16 || !labels || !templates || !score || !kept || !person || !cohesion || !summary) return "NULL rows, labels or output pointer";
    if (G <= 0 || dim <= 0 || dim > FID_TEMPLATE_MAX_DIM) return "G must be positive and dim 1 .. 4096";
    if (n <= 0 || n > FID_TEMPLATE_MAX_ROWS) return "n must be 1 .. 1048576";
    if (P <= 0 || P > n) return "P must be 1 .. n";
    if (!(min_score == min_score) || min_score - min_score != 0.f) return "min_score must be finite";
    return nullptr;
}

// rows == NULL: positions = gallery rows 0 .. G - 1 (the caller passes n = G); weights == NULL: every weight is 1.  Outputs: templates fp16
// [P, dim], score float [n], kept int32 [n], person int32 [P, 4], cohesion float [P], summary int64 [6].
inline void fid_templates_table_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, const int32_t *weights,
                                     int n, int P, float min_score, void *templates_f16, float *score, int32_t *kept, int32_t *person,
                                     float *cohesion, int64_t *summary) {
    const uint16_t *g = (const uint16_t *)rows_f16;
    uint16_t *tpl = (uint16_t *)templates_f16;
    std::vector<int32_t> start((size_t)P + 1, 0), list;
    int64_t took = 0, rejected = 0, dropped = 0, with_member = 0, zero = 0;
    for (int k = 0; k < n; k++) {
        const long long row = rows ? rows[k] : k;
        const int32_t label = labels[k], w = weights ? weights[k] : 1;
        kept[k] = -1;
        score[k] = 0.f;
        if (row < 0 || row >= G || label < 0 || label >= P || w < 1 || w > 255) continue;
        unsigned any = 0;
        bool ok = true;
        for (int c = 0; c < dim; c++) {
            const uint16_t h = g[(size_t)row * dim + c];
            any |= h & 0x7FFFu;
            ok = ok && fid_tpl_elem_ok(h);
        }
        if (!ok || !any) { rejected++; continue; }
        kept[k] = 1;                                // (a member; the decision follows)
        start[(size_t)label + 1]++;
        took++;
    }
    for (int p = 0; p < P; p++) start[(size_t)p + 1] += start[p];
    list.resize((size_t)took + 1);
    {
        std::vector<int32_t> at(start.begin(), start.end() - 1);
        for (int k = 0; k < n; k++)
            if (kept[k] == 1) list[(size_t)at[labels[k]]++] = k;
    }
    std::vector<int64_t> S((size_t)dim);
    std::vector<int32_t> T((size_t)dim);
    // the sum of the members of p whose kept word is 1, the template row of p from it; -> nrm, W
    auto make = [&](int p, int64_t &W) {
        for (int c = 0; c < dim; c++) S[c] = 0;
        W = 0;
        for (int32_t i = start[p]; i < start[(size_t)p + 1]; i++) {
            const int k = list[i];
            if (kept[k] != 1) continue;
            const int64_t w = weights ? weights[k] : 1;
            const uint16_t *x = g + (size_t)(rows ? rows[k] : k) * dim;
            for (int c = 0; c < dim; c++) S[c] += w * (int64_t)fid_tpl_fixed(x[c]);
            W += w;
        }
        const double nrm = fid_tpl_norm_host(S.data(), dim);
        for (int c = 0; c < dim; c++) tpl[(size_t)p * dim + c] = nrm > 0.0 ? fid_tpl_f32_to_f16(fid_tpl_element(S[c], nrm)) : (uint16_t)0;
        return nrm;
    };
    for (int p = 0; p < P; p++) {
        const int32_t members = start[(size_t)p + 1] - start[p];
        int64_t W = 0;
        double nrm = make(p, W);
        uint64_t low = ~0ull, high = 0ull;
        int32_t keeps = 0;
        for (int c = 0; c < dim; c++) T[c] = fid_tpl_fixed(tpl[(size_t)p * dim + c]);
        for (int32_t i = start[p]; i < start[(size_t)p + 1]; i++) {
            const int k = list[i];
            const uint16_t *x = g + (size_t)(rows ? rows[k] : k) * dim;
            int64_t D = 0;
            for (int c = 0; c < dim; c++) D += (int64_t)fid_tpl_fixed(x[c]) * (int64_t)T[c];
            score[k] = fid_tpl_score(D);
            uint32_t u;
            memcpy(&u, &score[k], 4);
            const uint64_t kl = fid_tpl_low_key(u, k), kh = fid_tpl_high_key(u, k);
            if (kl < low) low = kl;
            if (kh > high) high = kh;
            kept[k] = fid_tpl_keeps(score[k], min_score) ? 1 : 0;
            keeps += kept[k];
        }
        if (keeps != members) nrm = make(p, W);     // (with nothing dropped the final template is the first one)
        dropped += members - keeps;
        with_member += members > 0;
        zero += !(nrm > 0.0);
        cohesion[p] = fid_tpl_cohesion(nrm, W);
        person[(size_t)p * 4 + 0] = members;
        person[(size_t)p * 4 + 1] = keeps;
        person[(size_t)p * 4 + 2] = members ? (int32_t)(uint32_t)low : -1;
        person[(size_t)p * 4 + 3] = members ? (int32_t)~(uint32_t)high : -1;
    }
    summary[0] = took; summary[1] = with_member; summary[2] = zero; summary[3] = dropped; summary[4] = rejected; summary[5] = 0;
}
