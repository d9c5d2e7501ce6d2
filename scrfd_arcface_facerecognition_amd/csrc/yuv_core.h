// NV12 <-> BGR, once, for the device kernels (align.hip: fid_nv12_to_bgr, fid_bgr_to_nv12 and the fused letterbox, tile cut and warp;
// draw.hip: fid_draw_faces_nv12), the host twins (fid_nv12_to_bgr_host, fid_bgr_to_nv12_host, fid_draw_faces_nv12_host) and the stand-alone
// sanitizer drivers (tests/nv12_host_driver.cpp, tests/draw_nv12_host_driver.cpp): one (Y, U, V) sample -> one BGR pixel and back, the
// address of a pixel's samples in a pitched two-plane frame, and the check of a layout.  Integer arithmetic only, so device, host and a
// numpy restatement agree to the byte.  Plain inline functions, no HIP runtime call; compiles with a host-only compiler.
// The definition is include/faceid.h's (fid_nv12_to_bgr): the integer tables are written out there.  Nothing here is the reference's, which
// gets BGR frames from cv2.VideoCapture (main.py:174-184) and never sees the decoder's NV12.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_YHD __host__ __device__ inline
#else
#define FID_YHD inline
#endif

#define FID_YUV_SHIFT 20

// the five integers of a standard and its luma offset (a FID_YUV_*_TABLE of include/faceid.h)
struct fid_yuv_coeffs {
    int32_t cy, cub, cug, cvg, cvr, yoff;
};

// false: not one of the FID_YUV_* standards (k is left alone)
inline bool fid_yuv_coeffs_for(int standard, fid_yuv_coeffs *k) {
    static const fid_yuv_coeffs tab[3] = {FID_YUV_BT601_LIMITED_TABLE, FID_YUV_BT709_LIMITED_TABLE, FID_YUV_BT601_FULL_TABLE};
    if (standard < 0 || standard > 2) return false;
    *k = tab[standard];
    return true;
}

FID_YHD int fid_yuv_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One sample -> bgr[0 .. 2].  |yy| < 2^29 and every chroma term is below 2^28 in magnitude, so the sums stay inside int32; `>>` on a
// negative int is the arithmetic shift on every compiler this builds with (and by definition since C++20).
FID_YHD void fid_yuv_to_bgr(const fid_yuv_coeffs &k, int Y, int U, int V, int *bgr) {
    const int yy = (Y > k.yoff ? Y - k.yoff : 0) * k.cy, u = U - 128, v = V - 128, half = 1 << (FID_YUV_SHIFT - 1);
    bgr[0] = fid_yuv_sat8((yy + k.cub * u + half) >> FID_YUV_SHIFT);
    bgr[1] = fid_yuv_sat8((yy + k.cug * u + k.cvg * v + half) >> FID_YUV_SHIFT);
    bgr[2] = fid_yuv_sat8((yy + k.cvr * v + half) >> FID_YUV_SHIFT);
}

// Pixel (y, x) of the frame whose Y plane starts at yp and whose UV plane starts at uvp, rows `pitch` bytes apart: chroma is replicated,
// the sample of the 2 x 2 group the pixel lies in.  Reads yp[y*pitch + x] and uvp[(y>>1)*pitch + (x & ~1) + {0, 1}], nothing else.
FID_YHD void fid_nv12_pixel(const fid_yuv_coeffs &k, const uint8_t *yp, const uint8_t *uvp, int pitch, int y, int x, int *bgr) {
    const uint8_t *c = uvp + (size_t)(y >> 1) * (size_t)pitch + (size_t)(x & ~1);
    fid_yuv_to_bgr(k, yp[(size_t)y * (size_t)pitch + (size_t)x], c[0], c[1], bgr);
}

// ---- the forward direction (include/faceid.h, fid_bgr_to_nv12): BGR -> Y per pixel, (U, V) per 2 x 2 group from the sums of its four pixels ----
// the nine integers of a standard and its luma offset (a FID_YUV_*_FWD_TABLE of include/faceid.h)
struct fid_yuv_fwd {
    int32_t yb, yg, yr, ub, ug, ur, vb, vg, vr, yoff;
};

// false: not one of the FID_YUV_* standards (k is left alone)
inline bool fid_yuv_fwd_for(int standard, fid_yuv_fwd *k) {
    static const fid_yuv_fwd tab[3] = {FID_YUV_BT601_LIMITED_FWD_TABLE, FID_YUV_BT709_LIMITED_FWD_TABLE, FID_YUV_BT601_FULL_FWD_TABLE};
    if (standard < 0 || standard > 2) return false;
    *k = tab[standard];
    return true;
}

// A forward sample as the device returns it.  Two of them packed side by side -- (a >> n clamped) | (b >> n clamped) << 8, which is what every
// caller here does -- match the compiler's pattern for gfx950's v_ashr_pk_u8_i32, and the pattern takes the upper half of that instruction's
// result for zero while the instruction leaves it as it was: the bytes OR-ed in above bit 15 came out wrong (docs/FINDINGS.md, "NV12 output").
// The empty statement keeps each clamped value a value of its own; it costs no instruction.
FID_YHD int fid_yuv_sample(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// luma of one pixel.  The Y row sums to at most 2^20, so the sum stays below 255 * 2^20 + 2^24 + 2^19 < 2^29
FID_YHD int fid_yuv_luma(const fid_yuv_fwd &k, int b, int g, int r) {
    return fid_yuv_sample(fid_yuv_sat8((k.yb * b + k.yg * g + k.yr * r + (k.yoff << FID_YUV_SHIFT) + (1 << (FID_YUV_SHIFT - 1))) >> FID_YUV_SHIFT));
}

// chroma of one 2 x 2 group from the sums of its four pixels (0 .. 1020 each): uv[0] = U, uv[1] = V.  No |coefficient| exceeds 2^19, a row
// holds one positive entry or two negative ones that sum to its negative: |sum| <= 1020 * 2^19 + 2^29 + 2^21 < 1.08e9, inside int32
FID_YHD void fid_yuv_chroma(const fid_yuv_fwd &k, int sb, int sg, int sr, int *uv) {
    const int bias = (128 << (FID_YUV_SHIFT + 2)) + (1 << (FID_YUV_SHIFT + 1));
    uv[0] = fid_yuv_sample(fid_yuv_sat8((k.ub * sb + k.ug * sg + k.ur * sr + bias) >> (FID_YUV_SHIFT + 2)));
    uv[1] = fid_yuv_sample(fid_yuv_sat8((k.vb * sb + k.vg * sg + k.vr * sr + bias) >> (FID_YUV_SHIFT + 2)));
}

// one solid colour as an overlay paints it: yuv[0] = Y(c), yuv[1], yuv[2] = (U, V) of the flat group S = 4 * c
FID_YHD void fid_yuv_of_colour(const fid_yuv_fwd &k, int b, int g, int r, int *yuv) {
    yuv[0] = fid_yuv_luma(k, b, g, r);
    fid_yuv_chroma(k, 4 * b, 4 * g, 4 * r, yuv + 1);
}

// layout checks shared by every NV12 entry point; NULL = fine, else what is wrong
inline const char *fid_nv12_check(const fid_nv12_desc *d, int B, int H, int W) {
    if (!d) return "a NULL layout";
    if (B <= 0 || H <= 0 || W <= 0) return "B, H or W is not positive";
    if ((H & 1) || (W & 1)) return "H and W must be even";
    if (d->pitch < W) return "pitch below W";
    if (d->uv_offset < (int64_t)d->pitch * H) return "uv_offset below pitch * H: the planes overlap";
    if (d->frame_stride < d->uv_offset + (int64_t)d->pitch * (H / 2)) return "frame_stride below uv_offset + pitch * H / 2: the frames overlap";
    if (d->standard < 0 || d->standard > 2) return "an unknown standard";
    return nullptr;
}

// B frames in plain loops (the layout has passed fid_nv12_check): dense BGR [B,H,W,3]
inline void fid_nv12_to_bgr_frames_host(const uint8_t *nv12, const fid_nv12_desc *d, int B, int H, int W, uint8_t *bgr) {
    fid_yuv_coeffs k;
    if (!fid_yuv_coeffs_for(d->standard, &k)) return;
    for (int b = 0; b < B; b++) {
        const uint8_t *yp = nv12 + (size_t)b * (size_t)d->frame_stride, *uvp = yp + d->uv_offset;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int v[3];
                fid_nv12_pixel(k, yp, uvp, d->pitch, y, x, v);
                uint8_t *o = bgr + (((size_t)b * H + y) * W + x) * 3;
                o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
            }
    }
}

// B dense BGR frames [B,H,W,3] -> the layout d in plain loops (the layout has passed fid_nv12_check).  Writes the first W bytes of every Y row
// and of every UV row, nothing else.
inline void fid_bgr_to_nv12_frames_host(const uint8_t *bgr, int B, int H, int W, uint8_t *nv12, const fid_nv12_desc *d) {
    fid_yuv_fwd k;
    if (!fid_yuv_fwd_for(d->standard, &k)) return;
    for (int b = 0; b < B; b++) {
        uint8_t *yp = nv12 + (size_t)b * (size_t)d->frame_stride, *uvp = yp + d->uv_offset;
        const uint8_t *img = bgr + (size_t)b * H * W * 3;
        for (int y = 0; y < H; y += 2)
            for (int x = 0; x < W; x += 2) {
                int s[3] = {0, 0, 0};
                for (int dy = 0; dy < 2; dy++)
                    for (int dx = 0; dx < 2; dx++) {
                        const uint8_t *p = img + ((size_t)(y + dy) * W + x + dx) * 3;
                        yp[(size_t)(y + dy) * (size_t)d->pitch + (size_t)(x + dx)] = (uint8_t)fid_yuv_luma(k, p[0], p[1], p[2]);
                        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
                    }
                int uv[2];
                fid_yuv_chroma(k, s[0], s[1], s[2], uv);
                uint8_t *c = uvp + (size_t)(y >> 1) * (size_t)d->pitch + (size_t)x;
                c[0] = (uint8_t)uv[0]; c[1] = (uint8_t)uv[1];
            }
    }
}
