// Measured face quality (include/faceid.h, fid_face_measure): sharpness, exposure and pose of every aligned crop of a row table in one launch,
// behind the warp on the same stream, nothing read back.  The reference's blur and lighting scores read no pixel
// (smart_face_recognition.py:1145-1216, "simplified") and its pose angles have no producer; this is the project's own definition, with its
// arithmetic in measure_core.h, shared with the host twin fid_face_measure_host below.
//
// Byte work, one 256-thread workgroup per row, each byte of the crop read at most once:
//   load     the luma of rows 15 .. 96, columns 12 .. 99 (the 82 x 82 patch the window's Laplacian touches, widened to whole groups of four
//            pixels) into LDS, one byte per pixel.  Four pixels are 12 contiguous bytes at a multiple of 12 from the crop's first byte: three
//            dword loads when the crop pointer is dword-aligned (every row of a table then is: 37 632 % 4 == 0), byte loads otherwise.
//            21 648 of the crop's 37 632 bytes.
//   stencil  a thread takes four adjacent window pixels at a time: five LDS dwords (centre, left, right, up, down), integer sums in registers.
//   reduce   __shfl_down inside the wave (every per-wave sum fits 32 bits: 1 792 pixels x 1020^2 < 2^31), then the four waves' partial sums
//            through LDS into int64 (6 400 x 1020^2 does not fit 32 bits) by thread 0, which also finishes the fp64 part.
// Integer sums do not depend on the order of summation, so the device, the host loops and the numpy oracle agree word for word.
//
// This file must never get a fast-math flag: the derived words are specified with correctly rounded divides and square roots.
#include "common.h"
#include "measure_core.h"

namespace {

constexpr int PATCH_ROW0 = FID_MEASURE_LO - 1;                           // crop row of patch row 0
constexpr int PATCH_COL0 = 12;                                           // crop column of patch column 0 (a multiple of 4 below LO - 1)
constexpr int PATCH_ROWS = FID_MEASURE_HI - FID_MEASURE_LO + 2;          // 82
constexpr int PATCH_DW = 22;                                             // dwords per patch row: columns 12 .. 99
constexpr int WIN = FID_MEASURE_HI - FID_MEASURE_LO;                     // 80
constexpr int QUADS_X = WIN / 4;                                         // 20
static_assert(PATCH_COL0 % 4 == 0 && PATCH_COL0 + 4 == FID_MEASURE_LO && PATCH_COL0 + 4 * PATCH_DW >= FID_MEASURE_HI + 1 &&
              PATCH_COL0 + 4 * PATCH_DW <= FID_MEASURE_CROP, "the patch holds columns LO - 1 .. HI in whole groups of four inside the crop");

__device__ __forceinline__ uint32_t luma4(uint32_t d0, uint32_t d1, uint32_t d2) {
    const int y0 = fid_measure_luma(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
    const int y1 = fid_measure_luma(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
    const int y2 = fid_measure_luma((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
    const int y3 = fid_measure_luma((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
    return (uint32_t)y0 | ((uint32_t)y1 << 8) | ((uint32_t)y2 << 16) | ((uint32_t)y3 << 24);
}

__global__ void __launch_bounds__(256) face_measure(const uint8_t *__restrict__ crops, const float *__restrict__ kps,
                                                    const int32_t *__restrict__ src, const double *__restrict__ M,
                                                    int64_t *__restrict__ stats, float *__restrict__ measure) {
    __shared__ uint32_t s_y[PATCH_ROWS * PATCH_DW];
    __shared__ int32_t s_red[4][5];
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int face = src ? src[row] : (int)row;                          // (block-uniform; without a table the landmark row is the row itself)
    if (src && face < 0) {                                               // no face: 16 zero words, the crop is not read
        if (tid < 8) stats[row * 8 + tid] = 0;
        else if (tid < 16) measure[row * 8 + tid - 8] = 0.f;
        return;
    }
    const uint8_t *crop = crops + row * (size_t)(FID_MEASURE_CROP * FID_MEASURE_CROP * 3);
    const bool dwords = ((uintptr_t)crops & 3u) == 0u;
    for (int g = tid; g < PATCH_ROWS * PATCH_DW; g += 256) {
        const int r = g / PATCH_DW, q = g - r * PATCH_DW;
        const uint8_t *p = crop + ((PATCH_ROW0 + r) * FID_MEASURE_CROP + PATCH_COL0 + 4 * q) * 3;
        uint32_t d0, d1, d2;
        if (dwords) {
            const uint32_t *w = (const uint32_t *)p;
            d0 = w[0]; d1 = w[1]; d2 = w[2];
        } else {
            d0 = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            d1 = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
            d2 = (uint32_t)p[8] | ((uint32_t)p[9] << 8) | ((uint32_t)p[10] << 16) | ((uint32_t)p[11] << 24);
        }
        s_y[g] = luma4(d0, d1, d2);
    }
    __syncthreads();
    int sy = 0, syy = 0, sl = 0, sll = 0, clip = 0;                      // clip: n_dark | n_bright << 16
    for (int i = tid; i < WIN * QUADS_X; i += 256) {
        const int y = i / QUADS_X, xq = i - y * QUADS_X;
        const int at = (y + 1) * PATCH_DW + xq + 1;
        const uint32_t c = s_y[at], lf = s_y[at - 1], rt = s_y[at + 1], up = s_y[at - PATCH_DW], dn = s_y[at + PATCH_DW];
        const uint32_t lefts = (c << 8) | (lf >> 24), rights = (c >> 8) | (rt << 24);      // byte j: the left / right neighbour of pixel j
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int v = (int)((c >> (8 * j)) & 255u);
            const int lap = fid_measure_lap(v, (int)((lefts >> (8 * j)) & 255u), (int)((rights >> (8 * j)) & 255u),
                                            (int)((up >> (8 * j)) & 255u), (int)((dn >> (8 * j)) & 255u));
            sy += v; syy += v * v; sl += lap; sll += lap * lap;
            clip += (v <= FID_MEASURE_DARK ? 1 : 0) + (v >= FID_MEASURE_BRIGHT ? 1 << 16 : 0);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sy += __shfl_down(sy, off); syy += __shfl_down(syy, off); sl += __shfl_down(sl, off); sll += __shfl_down(sll, off);
        clip += __shfl_down(clip, off);
    }
    if ((tid & 63) == 0) {
        int32_t *o = s_red[tid >> 6];
        o[0] = sy; o[1] = syy; o[2] = sl; o[3] = sll; o[4] = clip;
    }
    __syncthreads();
    if (tid == 0) {
        fid_measure_sums s = {0, 0, 0, 0, 0, 0};
        for (int w = 0; w < 4; w++) {
            s.sy += s_red[w][0]; s.syy += s_red[w][1]; s.sl += s_red[w][2]; s.sll += s_red[w][3];
            s.n_dark += s_red[w][4] & 0xFFFF; s.n_bright += s_red[w][4] >> 16;
        }
        const bool pose = kps != nullptr && M != nullptr;
        fid_measure_row(&s, pose ? kps + (size_t)face * 10 : nullptr, pose ? M + row * 6 : nullptr, stats + row * 8, measure + row * 8);
    }
}

}  // namespace

extern "C" {

int fid_face_measure(fid_ctx *ctx, const uint8_t *crops_dev, int n_rows, const float *kps_dev, const int32_t *src_dev, const double *M_dev,
                     int64_t *stats_dev, float *measure_dev) {
    FID_REQUIRE(ctx, "measure: NULL context");
    const char *why = fid_measure_check(crops_dev, n_rows, kps_dev, M_dev, stats_dev, measure_dev);
    FID_REQUIRE(why == nullptr, "measure: %s", why ? why : "");
    if (n_rows == 0) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(face_measure, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, crops_dev, kps_dev, src_dev, M_dev, stats_dev, measure_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_face_measure_host(const uint8_t *crops, int n_rows, const float *kps, const int32_t *src, const double *M, int64_t *stats,
                          float *measure) {
    const char *why = fid_measure_check(crops, n_rows, kps, M, stats, measure);
    FID_REQUIRE(why == nullptr, "measure: %s", why ? why : "");
    fid_measure_table_host(crops, n_rows, kps, src, M, stats, measure);
    return FID_OK;
}

}  // extern "C"
