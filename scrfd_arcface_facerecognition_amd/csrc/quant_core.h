// The int8 quantisation rule of the coarse gallery scan, once, for the device kernels (coarse.hip), the host twin (fid_quantize_rows_i8_host)
// and the stand-alone sanitizer driver (tests/quant_host_driver.cpp).  Plain inline functions on bit patterns, no HIP runtime call; compiles with
// a host-only compiler.  The definition is include/faceid.h's (fid_quantize_rows_i8).
//
// One unit fp16 row u[0 .. dim):
//   m = max |u_j|.  m == 0, or any NaN / inf element: e = 0 and every code 0 (such a row scores 0 against everything: never a candidate).
//   otherwise e = the smallest integer with m <= 127 * 2^e, read from the exponent and mantissa bits of m (no logarithm);
//   code_j = rint(u_j * 2^-e), ties to even, in [-127, 127].  u_j * 2^-e is exact in fp32 for every fp16 value, subnormals included (a power-of-two
//   scaling of an 11-bit significand into [2^-34, 127]), so each element is rounded exactly once and nothing is left to the platform.
// The coarse score of (query q, row g) is ldexpf((float)dot_i32(code_q, code_g), e_q + e_g): |dot| <= dim * 127 * 127, below 2^24 for
// dim <= FID_QUANT_DIM_MAX, so the conversion to fp32 is exact; e lies in [-30, 10] (fp16's smallest subnormal 2^-24 .. its largest value 65504),
// so the scaled score is a normal fp32 number in [2^-60, 2^44) and the scaling is exact as well.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FID_QHD __host__ __device__ inline
#else
#define FID_QHD inline
#endif

#define FID_QUANT_DIM_MAX 1024
#define FID_QUANT_E_MIN (-30)
#define FID_QUANT_E_MAX 10
static_assert((long long)FID_QUANT_DIM_MAX * 127 * 127 < (1ll << 24), "an int8 dot product over dim <= FID_QUANT_DIM_MAX must be exact in fp32");

FID_QHD float fid_quant_bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
FID_QHD uint32_t fid_quant_float_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// an fp16 bit pattern as the fp32 number of the same value (finite inputs only; exact)
FID_QHD float fid_quant_half_value(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, fr = h & 0x3FFu;
    if (ex == 0) {                                                         // zero or subnormal: fr * 2^-24
        const float v = (float)fr * 5.9604644775390625e-08f;
        return sign ? -v : v;
    }
    return fid_quant_bits_to_float(sign | ((ex + 112u) << 23) | (fr << 13));
}
FID_QHD float fid_quant_pow2(int e) { return fid_quant_bits_to_float((uint32_t)(127 + e) << 23); }      // 2^e, -126 <= e <= 127

// max_abs_bits: the largest (bits & 0x7FFF) of the row (fp16 magnitudes order like their bit patterns); > 0x7BFF means a NaN or an inf
FID_QHD int fid_quant_row_exp(uint32_t max_abs_bits, bool *live) {
    *live = max_abs_bits != 0 && max_abs_bits <= 0x7BFFu;
    if (!*live) return 0;
    const uint32_t b = fid_quant_float_to_bits(fid_quant_half_value((uint16_t)max_abs_bits));
    // m = (1 + f / 2^23) * 2^x and 127 = (1 + 0x7E0000 / 2^23) * 2^6:  m <= 127 * 2^(x - 6) iff f <= 0x7E0000, else the next exponent
    return (int)(b >> 23) - 127 - 6 + ((b & 0x7FFFFFu) > 0x7E0000u ? 1 : 0);
}
FID_QHD int8_t fid_quant_code(uint16_t h, float inv_scale, bool live) {
    return live ? (int8_t)(int)rintf(fid_quant_half_value(h) * inv_scale) : (int8_t)0;
}

// exps[i], codes[i * dim ..] of n rows of unit_f16 [n, dim] (host arrays of exactly those sizes)
inline void fid_quantize_rows_i8_table_host(const uint16_t *unit_f16, int n, int dim, int8_t *codes, int8_t *exps) {
    for (size_t i = 0; i < (size_t)(n > 0 ? n : 0); i++) {
        const uint16_t *r = unit_f16 + i * dim;
        uint32_t mx = 0;
        for (int j = 0; j < dim; j++) mx = (r[j] & 0x7FFFu) > mx ? (r[j] & 0x7FFFu) : mx;
        bool live;
        const int e = fid_quant_row_exp(mx, &live);
        const float inv = fid_quant_pow2(-e);
        exps[i] = (int8_t)e;
        for (int j = 0; j < dim; j++) codes[i * dim + j] = fid_quant_code(r[j], inv, live);
    }
}
