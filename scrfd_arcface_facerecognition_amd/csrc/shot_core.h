// The best-shot score's arithmetic, once, for the device kernel (shots.hip), the host twin (fid_shot_score_host) and the stand-alone
// sanitizer driver (tests/shot_host_driver.cpp): one row of fid_face_measure's output -> one fp32 score.  The three terms are
// fid_face_gates_measured's blur, lighting and pose (gates.hip, quality5), from the same fid_measure_config fields.  Plain inline
// functions, no HIP runtime call; compiles with a host-only compiler.  The definition is include/faceid.h's (fid_shot_score).
//
// Every translation unit that includes this must be built with -ffp-contract=off and without any fast-math flag: every operation is
// rounded on its own and the divides are the correctly rounded ones.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_SHD __host__ __device__ inline
#else
#define FID_SHD inline
#endif

FID_SHD float fid_shot_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
FID_SHD float fid_shot_cap1(float x) { return x < 1.0f ? x : 1.0f; }       // python's min(1.0, x): 1 for a NaN

// flags: stats word 7 of the row; m: its 8 measure words
FID_SHD float fid_shot_score_row(int64_t flags, const float *m, float n_s, float n_c, float n_r) {
    if (!(flags & 1)) return -1.0f;                                        // no face, or no valid pixel part: never a candidate
    const float b = fid_shot_cap1(fid_shot_div(m[0], n_s));
    const float l = fid_shot_cap1(fid_shot_div(m[2], n_c)) * (1.0f - m[3]);
    float p = 0.0f;
    if (flags & 2) {
        const float x = 1.0f - fid_shot_div(m[6], n_r);
        p = x > 0.0f ? x : 0.0f;                                           // python's max(0.0, x)
    }
    const float s = (b * l) * p;
    return s == s ? s : __builtin_nanf("");                                // a NaN (from a NaN measure word) leaves as THE quiet NaN 0x7FC00000:
}                                                                          // IEEE 754 fixes neither sign nor payload, and hosts and devices differ

FID_SHD bool fid_shot_norm_ok(float v) { return v > 0.0f && v <= 3.4028234663852886e38f; }      // finite and > 0 (false for a NaN)

// argument checks shared by the device and the host entry point; NULL = fine, else what is wrong
inline const char *fid_shot_score_check(const void *stats, const void *measure, int n_rows, const fid_measure_config *c, const void *score) {
    if (n_rows < 0) return "n_rows is negative";
    if (!stats || !measure || !c || !score) return "a NULL stats, measure, config or score pointer";
    if (!fid_shot_norm_ok(c->sharpness_normalization) || !fid_shot_norm_ok(c->contrast_normalization) ||
        !fid_shot_norm_ok(c->residual_normalization))
        return "a normalisation that is not finite and > 0";
    return nullptr;
}

inline void fid_shot_score_table_host(const int64_t *stats, const float *measure, int n_rows, const fid_measure_config *c, float *score) {
    for (size_t i = 0; i < (size_t)(n_rows > 0 ? n_rows : 0); i++)
        score[i] = fid_shot_score_row(stats[i * 8 + 7], measure + i * 8, c->sharpness_normalization, c->contrast_normalization,
                                      c->residual_normalization);
}
