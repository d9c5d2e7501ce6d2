// The measured face quality's arithmetic, once, for the device kernel (measure.hip), the host twin (fid_face_measure_host) and the
// stand-alone sanitizer driver (tests/measure_host_driver.cpp): luma and Laplacian of one pixel, the integer sums -> four floats, the
// pose ratios from landmarks and the similarity matrix.  Plain inline functions, no HIP runtime call; compiles with a host-only compiler.
// The definition is include/faceid.h's (fid_face_measure); nothing here is the reference's, whose blur and lighting scores read no pixel
// (smart_face_recognition.py:1145-1216).
//
// Every translation unit that includes this must be built with -ffp-contract=off and without any fast-math flag: the pose part rounds every
// + - * / and square root separately, and the divides and square roots are the correctly rounded ones.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_MHD __host__ __device__ inline
#else
#define FID_MHD inline
#endif

#define FID_MEASURE_CROP 112                   // the aligned crop is 112 x 112 x 3, BGR
#define FID_MEASURE_LO 16                      // the window: LO <= x, y < HI
#define FID_MEASURE_HI 96
#define FID_MEASURE_N ((FID_MEASURE_HI - FID_MEASURE_LO) * (FID_MEASURE_HI - FID_MEASURE_LO))
#define FID_MEASURE_DARK 16                    // Y <= 16 counts as dark
#define FID_MEASURE_BRIGHT 239                 // Y >= 239 counts as bright
#define FID_MEASURE_PIXELS_VALID 1
#define FID_MEASURE_POSE_VALID 2

// the ArcFace template of align.hip: float32 values, widened to double where they are used
#define FID_MEASURE_TEMPLATE_INIT {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f}

// the integer sums over the window: stats words 1 .. 6
struct fid_measure_sums {
    int64_t sy, syy, sl, sll, n_dark, n_bright;
};

FID_MHD int fid_measure_luma(int b, int g, int r) { return (29 * b + 150 * g + 77 * r + 128) >> 8; }
FID_MHD int fid_measure_lap(int c, int left, int right, int up, int down) { return 4 * c - left - right - up - down; }

// one window pixel into the sums (c: its luma, lap: its Laplacian)
FID_MHD void fid_measure_add(fid_measure_sums *s, int c, int lap) {
    s->sy += c; s->syy += (int64_t)c * c; s->sl += lap; s->sll += (int64_t)lap * lap;
    s->n_dark += c <= FID_MEASURE_DARK; s->n_bright += c >= FID_MEASURE_BRIGHT;
}

// the sums of one crop in plain loops: what the kernel's workgroup computes together
FID_MHD void fid_measure_crop_sums(const uint8_t *crop, fid_measure_sums *s) {
    s->sy = s->syy = s->sl = s->sll = s->n_dark = s->n_bright = 0;
    for (int y = FID_MEASURE_LO; y < FID_MEASURE_HI; y++)
        for (int x = FID_MEASURE_LO; x < FID_MEASURE_HI; x++) {
            const uint8_t *p = crop + ((size_t)y * FID_MEASURE_CROP + x) * 3;
            const uint8_t *l = p - 3, *r = p + 3, *u = p - FID_MEASURE_CROP * 3, *d = p + FID_MEASURE_CROP * 3;
            const int c = fid_measure_luma(p[0], p[1], p[2]);
            fid_measure_add(s, c, fid_measure_lap(c, fid_measure_luma(l[0], l[1], l[2]), fid_measure_luma(r[0], r[1], r[2]),
                                                  fid_measure_luma(u[0], u[1], u[2]), fid_measure_luma(d[0], d[1], d[2])));
        }
}

// sums -> measure[0 .. 3]: each integer expression in int64, converted once to double (exact: below 2^53), one correctly rounded divide
// (and square root), one rounding to fp32
FID_MHD void fid_measure_finish(const fid_measure_sums *s, float *m) {
    const int64_t N = FID_MEASURE_N;
    const double nn = (double)(N * N);
    m[0] = (float)((double)(N * s->sll - s->sl * s->sl) / nn);
    m[1] = (float)((double)s->sy / (double)N);
    m[2] = (float)sqrt((double)(N * s->syy - s->sy * s->sy) / nn);
    m[3] = (float)((double)(s->n_dark + s->n_bright) / (double)N);
}

FID_MHD bool fid_measure_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }       // false for a NaN
FID_MHD bool fid_measure_finitef(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// Ry / Rp of a point set q[10] (include/faceid.h); *w and *h: the eye distance and the eye-to-mouth height they divide by
FID_MHD void fid_measure_ratios(const double *q, double *ry, double *rp, double *w, double *h) {
    const double ex = (q[0] + q[2]) / 2.0, ey = (q[1] + q[3]) / 2.0;
    const double mx = (q[6] + q[8]) / 2.0, my = (q[7] + q[9]) / 2.0;
    *w = q[2] - q[0];
    *h = my - ey;
    *ry = (q[4] - (ex + mx) / 2.0) / *w;
    *rp = (q[5] - ey) / *h;
}

// landmarks k[10] (float32) and M[6] -> out[0 .. 2] = yaw, pitch, residual; false (and three zeros) when the pose part is not valid
FID_MHD bool fid_measure_pose(const float *k, const double *M, float *out) {
    const float tf[10] = FID_MEASURE_TEMPLATE_INIT;
    out[0] = out[1] = out[2] = 0.f;
    for (int i = 0; i < 6; i++)
        if (!fid_measure_finite(M[i])) return false;
    double p[10], t[10], ss = 0.0;
    for (int i = 0; i < 5; i++) {
        const double kx = (double)k[2 * i], ky = (double)k[2 * i + 1];
        p[2 * i] = (M[0] * kx + M[1] * ky) + M[2];
        p[2 * i + 1] = (M[3] * kx + M[4] * ky) + M[5];
        t[2 * i] = (double)tf[2 * i]; t[2 * i + 1] = (double)tf[2 * i + 1];
        const double dx = p[2 * i] - t[2 * i], dy = p[2 * i + 1] - t[2 * i + 1];
        ss = ss + (dx * dx + dy * dy);
    }
    double ryp, rpp, w, h, ryt, rpt, wt, ht;
    fid_measure_ratios(p, &ryp, &rpp, &w, &h);
    fid_measure_ratios(t, &ryt, &rpt, &wt, &ht);
    if (!(w > 0.0 && h > 0.0)) return false;
    const float yaw = (float)(ryp - ryt), pitch = (float)(rpp - rpt), res = (float)sqrt(ss / 5.0);
    if (!(fid_measure_finitef(yaw) && fid_measure_finitef(pitch) && fid_measure_finitef(res))) return false;
    out[0] = yaw; out[1] = pitch; out[2] = res;
    return true;
}

// the 16 output words of one face row from its sums; k / M: NULL = pixel part only
FID_MHD void fid_measure_row(const fid_measure_sums *s, const float *k, const double *M, int64_t *stats, float *measure) {
    int64_t flags = FID_MEASURE_PIXELS_VALID;
    fid_measure_finish(s, measure);
    measure[4] = measure[5] = measure[6] = measure[7] = 0.f;
    if (k && M && fid_measure_pose(k, M, measure + 4)) flags |= FID_MEASURE_POSE_VALID;
    stats[0] = FID_MEASURE_N; stats[1] = s->sy; stats[2] = s->syy; stats[3] = s->sl; stats[4] = s->sll;
    stats[5] = s->n_dark; stats[6] = s->n_bright; stats[7] = flags;
}

// argument checks shared by the device and the host entry point; NULL = fine, else what is wrong
inline const char *fid_measure_check(const void *crops, int n_rows, const void *kps, const void *M, const void *stats, const void *measure) {
    if (n_rows < 0) return "n_rows is negative";
    if (!crops || !stats || !measure) return "a NULL crops, stats or measure pointer";
    if ((kps == nullptr) != (M == nullptr)) return "landmarks and M come together or not at all";
    return nullptr;
}

// the whole table in plain loops on host arrays: fid_face_measure_host, and what the stand-alone driver runs
inline void fid_measure_table_host(const uint8_t *crops, int n_rows, const float *kps, const int32_t *src, const double *M, int64_t *stats,
                                   float *measure) {
    for (size_t row = 0; row < (size_t)(n_rows > 0 ? n_rows : 0); row++) {
        if (src && src[row] < 0) {                                            // no face: the crop is not read
            for (int i = 0; i < 8; i++) { stats[row * 8 + i] = 0; measure[row * 8 + i] = 0.f; }
            continue;
        }
        const size_t face = src ? (size_t)src[row] : row;
        fid_measure_sums s;
        fid_measure_crop_sums(crops + row * (size_t)(FID_MEASURE_CROP * FID_MEASURE_CROP * 3), &s);
        fid_measure_row(&s, kps ? kps + face * 10 : nullptr, M ? M + row * 6 : nullptr, stats + row * 8, measure + row * 8);
    }
}
