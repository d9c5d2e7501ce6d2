// 5-point alignment: Umeyama similarity estimate + fixed-point bilinear affine warp to 112x112.
// Replaces skimage SimilarityTransform.estimate and cv2.warpAffine as called by reference
// utils/helpers.py:18-59 (estimate_norm, norm_crop_image), reached from models/arcface.py:54-57.
//
//  * the estimate is the closed form of the 2-D Umeyama solution: with
//    A = dst_d^T src_d / n,  a = A00 + A11,  b = A10 - A01:  scale*R = [[a,-b],[b,a]] / var(src).
//    (The SVD form in skimage reduces to this for every rank >= 1 case, reflected inputs included,
//    because a reflection component has zero trace against any rotation.)  Evaluated in fp64 from
//    the fp32 landmarks; skimage itself runs the SVD in fp32, so agreement is ~1e-6 relative.
//  * the warp follows OpenCV's u8 INTER_LINEAR / BORDER_CONSTANT fixed-point path:
//    1/1024 coordinate grid, 1/32-pixel interpolation table, round-half-even cvRound.
//
// HBM-bound byte work: 37.6 KB written per face, <= 4 x 37.6 KB gathered from the frame (mostly L2).
#include "common.h"
#include "yuv_core.h"

namespace {

// Where a kernel's source pixels come from: load(y, x, v) gives pixel (y, x) of one image as three ints B, G, R.  The sampling arithmetic
// below (align_face_rows, letterbox_pixel) is written once over this; it only ever asks for pixels inside the image.
// BgrSrc: dense BGR bytes, rows `ld` pixels apart (W for a whole image, the frame's width for a rectangle of a frame).
struct BgrSrc {
    const uint8_t *p;
    int ld;
    __device__ __forceinline__ void load(int y, int x, int (&v)[3]) const {
        const uint8_t *q = p + ((size_t)y * ld + x) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    }
};
// Nv12Src: one NV12 frame (yuv_core.h), or the rectangle of it whose top-left pixel is (x0, y0): the chroma sample is the one of the
// FRAME's 2 x 2 grid, whatever the parity of the origin.  Every tap is converted here, before anything is interpolated.
struct Nv12Src {
    const uint8_t *yp, *uvp;
    int pitch, x0, y0;
    fid_yuv_coeffs k;
    __device__ __forceinline__ void load(int y, int x, int (&v)[3]) const { fid_nv12_pixel(k, yp, uvp, pitch, y0 + y, x0 + x, v); }
};

// A batch of frames as a by-value kernel argument: frame(b) gives image b's source and its size, frame(b, x0, y0) the part of it whose
// top-left pixel is (x0, y0).  The kernels below are written once over these.
template <class Src>
struct Frame {
    Src src;
    int H, W;
};
struct BgrBatch {            // dense uint8 [B, H, W, 3]
    const uint8_t *p;
    int H, W;
    __device__ __forceinline__ Frame<BgrSrc> frame(int b, int x0 = 0, int y0 = 0) const {
        return {BgrSrc{p + (((size_t)b * H + y0) * W + x0) * 3, W}, H, W};
    }
};
struct RaggedBatch {         // mixed sizes: image b's base, H and W from the per-image table (block-uniform index: the entry stays in scalar registers)
    const uint8_t *p;
    const fid::RaggedImg *tab;   // (the host's entries until upload_table has run)
    __device__ __forceinline__ Frame<BgrSrc> frame(int b) const {
        const fid::RaggedImg g = tab[b];
        return {BgrSrc{p + g.off, g.W}, g.H, g.W};
    }
};
struct Nv12Batch {           // fid_nv12_desc with the standard's integers resolved on the host
    const uint8_t *p;
    long long frame_stride, uv_offset;
    int pitch;
    fid_yuv_coeffs k;
    int H, W;
    __device__ __forceinline__ Frame<Nv12Src> frame(int b, int x0 = 0, int y0 = 0) const {
        const uint8_t *f = p + (size_t)b * (size_t)frame_stride;
        return {Nv12Src{f, f + uv_offset, pitch, x0, y0, k}, H, W};
    }
};

__constant__ double c_template[10] = {38.2946, 51.6963, 73.5318, 51.5014, 56.0252, 71.7366, 41.5493, 92.3655, 70.7299, 92.2041};

__device__ __forceinline__ long long cv_round(double v) {
    // cvRound == lrint (round half to even); saturate_cast<int> semantics for out-of-range / NaN
    if (!(v > -2147483648.0)) return -2147483648ll;
    if (!(v < 2147483647.0)) return 2147483647ll;
    return __double2ll_rn(v);
}

constexpr int OUT = 112;
constexpr int ROWS_PER_BLOCK = 16;

// One block's share (ROWS_PER_BLOCK output rows from y0) of one face's crop: thread 0 estimates the transform from the landmarks `lm`
// (NULL = no face: zero crop, zero M), every thread warps.  `src` = the face's frame, `dst` = its crop, `mo` = its row of M_out (or NULL).
// An NV12 source converts its taps before they are weighted.
template <class Src>
__device__ __forceinline__ void align_face_rows(const Src &src, int H, int W, const float *lm, uint8_t *dst, double *mo, int y0) {
    const bool valid = lm != nullptr;
    __shared__ double sm[6];  // inverse map m00 m01 m02 m10 m11 m12
    __shared__ int ok;
    if (threadIdx.x == 0) {
        ok = 0;
        if (valid) {
            // c_template holds the float32 template values widened to double, like skimage sees them
            double sx[5], sy[5], dx[5], dy[5], msx = 0, msy = 0, mdx = 0, mdy = 0;
            for (int i = 0; i < 5; i++) {
                sx[i] = (double)lm[2 * i]; sy[i] = (double)lm[2 * i + 1];
                dx[i] = (double)(float)c_template[2 * i]; dy[i] = (double)(float)c_template[2 * i + 1];
                msx += sx[i]; msy += sy[i]; mdx += dx[i]; mdy += dy[i];
            }
            msx /= 5; msy /= 5; mdx /= 5; mdy /= 5;
            double a = 0, bb = 0, var = 0;
            for (int i = 0; i < 5; i++) {
                const double px = sx[i] - msx, py = sy[i] - msy, qx = dx[i] - mdx, qy = dy[i] - mdy;
                a += qx * px + qy * py;   // n * (A00 + A11)
                bb += qy * px - qx * py;  // n * (A10 - A01)
                var += px * px + py * py; // n * var
            }
            const double M00 = a / var, M01 = -bb / var, M10 = bb / var, M11 = a / var;
            const double M02 = mdx - (M00 * msx + M01 * msy), M12 = mdy - (M10 * msx + M11 * msy);
            if (mo) {
                mo[0] = M00; mo[1] = M01; mo[2] = M02; mo[3] = M10; mo[4] = M11; mo[5] = M12;
            }
            // cv2.warpAffine inverts M (no WARP_INVERSE_MAP flag)
            double D = M00 * M11 - M01 * M10;
            D = D != 0 ? 1.0 / D : 0.0;
            const double A11 = M11 * D, A22 = M00 * D;
            const double m00 = A11, m01 = -M01 * D, m10 = -M10 * D, m11 = A22;
            sm[0] = m00; sm[1] = m01; sm[2] = -m00 * M02 - m01 * M12;
            sm[3] = m10; sm[4] = m11; sm[5] = -m10 * M02 - m11 * M12;
            ok = isfinite(M00) && isfinite(M01) && isfinite(M02) && isfinite(M12);
        } else if (mo && y0 == 0) {
            for (int i = 0; i < 6; i++) mo[i] = 0.0;
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < ROWS_PER_BLOCK * OUT; p += blockDim.x) {
        const int y = y0 + p / OUT, x = p % OUT;
        uint8_t *o = dst + ((size_t)y * OUT + x) * 3;
        if (!ok) { o[0] = o[1] = o[2] = 0; continue; }
        const long long X0 = cv_round((sm[1] * y + sm[2]) * 1024.0) + 16;
        const long long Y0 = cv_round((sm[4] * y + sm[5]) * 1024.0) + 16;
        const long long ad = cv_round(sm[0] * x * 1024.0), bd = cv_round(sm[3] * x * 1024.0);
        const long long X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
        long long sxl = X >> 5, syl = Y >> 5;
        sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);  // saturate_cast<short>
        syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
        const int ix = (int)sxl, iy = (int)syl, fx = (int)(X & 31), fy = (int)(Y & 31);
        const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
        const bool x0in = ix >= 0 && ix < W, x1in = ix + 1 >= 0 && ix + 1 < W;
        const bool y0in = iy >= 0 && iy < H, y1in = iy + 1 >= 0 && iy + 1 < H;
        int acc[3] = {512, 512, 512};
        int q[3];
        if (y0in && x0in) { src.load(iy, ix, q); acc[0] += w00 * q[0]; acc[1] += w00 * q[1]; acc[2] += w00 * q[2]; }
        if (y0in && x1in) { src.load(iy, ix + 1, q); acc[0] += w01 * q[0]; acc[1] += w01 * q[1]; acc[2] += w01 * q[2]; }
        if (y1in && x0in) { src.load(iy + 1, ix, q); acc[0] += w10 * q[0]; acc[1] += w10 * q[1]; acc[2] += w10 * q[2]; }
        if (y1in && x1in) { src.load(iy + 1, ix + 1, q); acc[0] += w11 * q[0]; acc[1] += w11 * q[1]; acc[2] += w11 * q[2]; }
        o[0] = (uint8_t)(acc[0] >> 10); o[1] = (uint8_t)(acc[1] >> 10); o[2] = (uint8_t)(acc[2] >> 10);
    }
}

// Which face output row blockIdx.y holds: its frame, its row of the post-process's landmark array (face b * cap + f), and whether there is one.
struct FaceRow {
    int b;
    size_t lm;
    bool valid;
};
struct SlotRows {            // B x F face slots: row b * F + f is face f of frame b, empty from counts[b] on
    const int *counts;
    int cap, F;
    __device__ __forceinline__ FaceRow at(int slot) const {
        const int b = slot / F, f = slot - b * F;
        return {b, (size_t)b * cap + f, f < counts[b] && f < cap};
    }
};
// a dense row table (fid_face_pack): row i holds face src_rows[i] = b * cap + f, or -1 = no face (reference main.py:130-134 embeds every
// face models/scrfd.py:159-177 returned; the table lists them without per-frame padding)
struct PackedRows {
    const int *src_rows;
    int B, cap;
    __device__ __forceinline__ FaceRow at(int row) const {
        const int s = src_rows[row];
        const bool valid = s >= 0 && s < B * cap;
        return {valid ? s / cap : 0, (size_t)s, valid};
    }
};

template <class Frames, class Rows>
__global__ void __launch_bounds__(256) align_warp(Frames frames, Rows rows, const float *kps, uint8_t *crops, double *M_out) {
    const FaceRow r = rows.at(blockIdx.y);
    const auto f = frames.frame(r.b);
    align_face_rows(f.src, f.H, f.W, r.valid ? kps + r.lm * 10 : nullptr, crops + (size_t)blockIdx.y * OUT * OUT * 3,
                    M_out ? M_out + (size_t)blockIdx.y * 6 : nullptr, blockIdx.x * ROWS_PER_BLOCK);
}

// cv2.resize's INTER_LINEAR rule for output coordinate d of an axis with n source pixels: the two taps s0, s1 and their 11-bit weights a0, a1
__device__ __forceinline__ void resize_coeff(int d, double scale, int n, int &s0, int &s1, int &a0, int &a1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    s0 = s; s1 = min(s + 1, n - 1);
    a1 = (int)rintf(__fmul_rn(f, 2048.f));
    a0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
}

// the 12 bytes of four BGR pixels as three dwords
__device__ __forceinline__ void store_quad(const uint8_t (&px)[12], unsigned *o) {
#pragma unroll
    for (int j = 0; j < 3; j++)
        o[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
}

// cv2.resize INTER_LINEAR u8 + zero letterbox paste (scrfd.py:135-138): output pixel (x, y) of one image, written to o.
// `src` is the H x W image (a dense image, or a rectangle of a frame for fid_tile_cut); an NV12 source converts each of the pixels asked for below.
template <class Src>
__device__ __forceinline__ void letterbox_pixel(const Src &src, int H, int W, uint8_t *o, int x, int y, int new_h, int new_w,
                                                double scale_x, double scale_y, int area2x) {
    if (x >= new_w || y >= new_h) { o[0] = o[1] = o[2] = 0; return; }
    int p00[3], p01[3], p10[3], p11[3];
    if (new_w == W && new_h == H) {
        src.load(y, x, p00);
        o[0] = (uint8_t)p00[0]; o[1] = (uint8_t)p00[1]; o[2] = (uint8_t)p00[2];
        return;
    }
    if (area2x) {  // exact 2x decimation is INTER_AREA inside cv2.resize
        src.load(2 * y, 2 * x, p00); src.load(2 * y, 2 * x + 1, p01);
        src.load(2 * y + 1, 2 * x, p10); src.load(2 * y + 1, 2 * x + 1, p11);
        for (int c = 0; c < 3; c++) o[c] = (uint8_t)((p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2);
        return;
    }
    int sx0, sx1, a0, a1, sy0, sy1, b0, b1;
    resize_coeff(x, scale_x, W, sx0, sx1, a0, a1);
    resize_coeff(y, scale_y, H, sy0, sy1, b0, b1);
    src.load(sy0, sx0, p00); src.load(sy0, sx1, p01);
    src.load(sy1, sx0, p10); src.load(sy1, sx1, p11);
    for (int c = 0; c < 3; c++) {
        const int T0 = p00[c] * a0 + p01[c] * a1;
        const int T1 = p10[c] * a0 + p11[c] * a1;
        int v = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2;
        o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// FOUR consecutive output pixels of row y through letterbox_pixel, leaving as three aligned dwords (in_w % 4 == 0, o 4-byte aligned): the same
// bytes by construction.  For sources letterbox_pixels4 below cannot read (it fetches BGR words).  The NV12 tile cut uses it: 288 tiles of 1080p
// frames 0.41 -> 0.29 ms, the byte stores of the native tiles being what the one-pixel kernel waits for (docs/FINDINGS.md).
template <class Src>
__device__ __forceinline__ void letterbox_quad(const Src &src, int H, int W, unsigned *o, int x4, int y, int new_h, int new_w, double scale_x,
                                               double scale_y, int area2x) {
    uint8_t px[12];
#pragma unroll
    for (int i = 0; i < 4; i++) letterbox_pixel(src, H, W, px + 3 * i, x4 + i, y, new_h, new_w, scale_x, scale_y, area2x);
    store_quad(px, o);
}

// Where the one-pixel kernel's image blockIdx.z and its letterbox geometry come from: pixel(frames, z, o, x, y) writes output pixel (x, y).
struct UniformGeom {         // every image of the batch alike: the geometry travels as kernel arguments
    int new_h, new_w;
    double scale_x, scale_y;
    int area2x;
    template <class Frames>
    __device__ __forceinline__ void pixel(const Frames &frames, int b, uint8_t *o, int x, int y) const {
        const auto f = frames.frame(b);
        letterbox_pixel(f.src, f.H, f.W, o, x, y, new_h, new_w, scale_x, scale_y, area2x);
    }
};
struct RaggedGeom {          // a mixed-size batch: the image's entry of the batch's table; identity and exact-2x are decided per image
    __device__ __forceinline__ void pixel(const RaggedBatch &frames, int b, uint8_t *o, int x, int y) const {
        const fid::RaggedImg g = frames.tab[b];
        letterbox_pixel(BgrSrc{frames.p + g.off, g.W}, g.H, g.W, o, x, y, g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2);
    }
};
// Tile t of the table (fid_tile_cut), cut from its frame.  The rectangle's pixels are addressed in FRAME coordinates, so an odd (x0, y0)
// keeps an NV12 frame's chroma grid.  (kind 0: new_h x new_w == h x w, which letterbox_pixel copies 1:1 and pads with zeros)
struct TileGeom {
    const fid::TileEntry *tab;
    template <class Frames>
    __device__ __forceinline__ void pixel(const Frames &frames, int t, uint8_t *o, int x, int y) const {
        const fid::TileEntry g = tab[t];
        letterbox_pixel(frames.frame(g.frame, g.x0, g.y0).src, g.h, g.w, o, x, y, g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2);
    }
};

// one output pixel per thread: image (or tile) blockIdx.z into its own in_h x in_w detector input
template <class Frames, class Geom>
__global__ void __launch_bounds__(256) letterbox_kernel(Frames frames, Geom geom, uint8_t *out, int in_h, int in_w) {
    const int z = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= in_w) return;
    geom.pixel(frames, z, out + (((size_t)z * in_h + y) * in_w + x) * 3, x, y);
}

// fid_nv12_to_bgr: two horizontally adjacent pixels per thread (they share one chroma sample), dense BGR out
__global__ void __launch_bounds__(256) nv12_to_bgr_kernel(Nv12Batch nv, uint8_t *out) {
    const int b = blockIdx.z, H = nv.H, W = nv.W;
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2, y = blockIdx.y;
    if (x >= W) return;
    const Nv12Src s = nv.frame(b).src;
    const uint8_t *yr = s.yp + (size_t)y * s.pitch + x, *c = s.uvp + (size_t)(y >> 1) * s.pitch + x;      // (x is even: the pair's own sample)
    int v0[3], v1[3];
    fid_yuv_to_bgr(s.k, yr[0], c[0], c[1], v0);
    fid_yuv_to_bgr(s.k, yr[1], c[0], c[1], v1);
    uint8_t *o = out + (((size_t)b * H + y) * W + x) * 3;
    o[0] = (uint8_t)v0[0]; o[1] = (uint8_t)v0[1]; o[2] = (uint8_t)v0[2];
    o[3] = (uint8_t)v1[0]; o[4] = (uint8_t)v1[1]; o[5] = (uint8_t)v1[2];
}

// fid_bgr_to_nv12: a thread owns two horizontally adjacent 2 x 2 groups -- four pixels of two rows; the last thread of a row whose W is no
// multiple of 4 owns one.  Both groups in a layout of dwords (`wide`: W % 4 == 0, every base and stride a multiple of 4): six dword loads,
// one dword of Y per row and one dword holding both (U, V) pairs; anything else moves the same bytes one by one.  Only the first W bytes of
// a row are ever addressed.
struct Nv12Out {
    uint8_t *p;
    long long frame_stride, uv_offset;
    int pitch;
    fid_yuv_fwd k;
};

__global__ void __launch_bounds__(256) bgr_to_nv12_kernel(const uint8_t *__restrict__ bgr, int H, int W, int quads, int per_frame, Nv12Out o,
                                                          int wide) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= per_frame) return;
    const int gy = i / quads, x = (i - gy * quads) * 4, y = gy * 2;
    const int npx = min(4, W - x);                                     // 4 or 2
    const uint8_t *src = bgr + (((size_t)b * H + y) * W + x) * 3;
    uint8_t *yp = o.p + (size_t)b * (size_t)o.frame_stride + (size_t)y * o.pitch + x;
    uint8_t *uvp = o.p + (size_t)b * (size_t)o.frame_stride + (size_t)o.uv_offset + (size_t)gy * o.pitch + x;
    uint32_t w[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};                   // the 12 bytes of each row's four pixels
    if (wide) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t *q = (const uint32_t *)(src + (size_t)r * W * 3);
            w[r][0] = q[0]; w[r][1] = q[1]; w[r][2] = q[2];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int k = 0; k < 12; k++)
                if (k < npx * 3) w[r][k >> 2] |= (uint32_t)src[(size_t)r * W * 3 + k] << (8 * (k & 3));
    }
    uint32_t yw[2] = {0u, 0u}, uvw = 0u;
#pragma unroll
    for (int g = 0; g < 2; g++) {
        int s[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int d = 0; d < 2; d++) {
                int c[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int k = (g * 2 + d) * 3 + ch;
                    c[ch] = (int)((w[r][k >> 2] >> (8 * (k & 3))) & 255u);
                }
                yw[r] |= (uint32_t)fid_yuv_luma(o.k, c[0], c[1], c[2]) << (8 * (g * 2 + d));
                s[0] += c[0]; s[1] += c[1]; s[2] += c[2];
            }
        int uv[2];
        fid_yuv_chroma(o.k, s[0], s[1], s[2], uv);
        uvw |= ((uint32_t)uv[0] | ((uint32_t)uv[1] << 8)) << (16 * g);
    }
    if (wide) {
        *(uint32_t *)yp = yw[0];
        *(uint32_t *)(yp + o.pitch) = yw[1];
        *(uint32_t *)uvp = uvw;
    } else {
        for (int k = 0; k < npx; k++) {
            yp[k] = (uint8_t)(yw[0] >> (8 * k));
            yp[(size_t)o.pitch + k] = (uint8_t)(yw[1] >> (8 * k));
            uvp[k] = (uint8_t)(uvw >> (8 * k));
        }
    }
}

// letterbox_pixel's bilinear arithmetic, FOUR consecutive output pixels per thread (in_w % 4 == 0): a source pixel is one unaligned 4-byte load
// instead of three 1-byte loads and the 12 output bytes leave as three aligned dwords -- 16 + 3 memory instructions per 4 pixels instead of 48 + 12
// (32 frames of 1080p -> 640x640: cfg 5 step 1.548 -> 1.535 ms).  `src_bytes` = bytes of the whole frame batch: the last pixel of the batch is read bytewise.
// letterbox_pixels4: output pixels x4 .. x4+3 of row y of the image whose first byte is frames[fbase] (rows `ld` pixels apart), as three dwords at o.
__device__ __forceinline__ void letterbox_pixels4(const uint8_t *frames, size_t fbase, int H, int W, int ld, unsigned *o, int x4, int y, int new_h, int new_w,
                                                  double scale_x, double scale_y, size_t src_bytes) {
    uint8_t px[12];
    auto fetch = [&](size_t off) -> unsigned {                  // the 3 bytes of a source pixel (byte 3 of the word is ignored)
        if (off + 4 <= src_bytes) {
            unsigned v;
            __builtin_memcpy(&v, frames + off, 4);
            return v;
        }
        return (unsigned)frames[off] | ((unsigned)frames[off + 1] << 8) | ((unsigned)frames[off + 2] << 16);
    };
    int sy0 = 0, sy1 = 0, b0 = 0, b1 = 0;
    if (y < new_h) resize_coeff(y, scale_y, H, sy0, sy1, b0, b1);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = x4 + i;
        if (x >= new_w || y >= new_h) { px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = 0; continue; }
        int sx0, sx1, a0, a1;
        resize_coeff(x, scale_x, W, sx0, sx1, a0, a1);
        const unsigned p00 = fetch(fbase + ((size_t)sy0 * ld + sx0) * 3), p01 = fetch(fbase + ((size_t)sy0 * ld + sx1) * 3);
        const unsigned p10 = fetch(fbase + ((size_t)sy1 * ld + sx0) * 3), p11 = fetch(fbase + ((size_t)sy1 * ld + sx1) * 3);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int T0 = (int)((p00 >> (8 * c)) & 255u) * a0 + (int)((p01 >> (8 * c)) & 255u) * a1;
            const int T1 = (int)((p10 >> (8 * c)) & 255u) * a0 + (int)((p11 >> (8 * c)) & 255u) * a1;
            const int v = (((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2;
            px[3 * i + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
    store_quad(px, o);
}

__global__ void __launch_bounds__(256) letterbox_kernel4(const uint8_t *frames, int H, int W, uint8_t *out, int in_h, int in_w, int new_h, int new_w,
                                                         double scale_x, double scale_y, size_t src_bytes) {
    const int b = blockIdx.z;
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= in_w) return;
    letterbox_pixels4(frames, (size_t)b * H * W * 3, H, W, W, (unsigned *)(out + (((size_t)b * in_h + y) * in_w + x4) * 3), x4, y, new_h, new_w,
                      scale_x, scale_y, src_bytes);
}

// a mixed-size batch, four pixels per thread; `src_bytes` = bytes of the caller's whole allocation (the guard of the 4-byte fetch).  An image
// that is copied (identity) or decimated by exactly 2 (INTER_AREA) takes letterbox_pixel for its four pixels: the branch is block-uniform.
__global__ void __launch_bounds__(256) letterbox_kernel4_ragged(const uint8_t *frames, const fid::RaggedImg *tab, uint8_t *out, int in_h, int in_w,
                                                                size_t src_bytes) {
    const int b = blockIdx.z;
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= in_w) return;
    const fid::RaggedImg g = tab[b];
    uint8_t *o = out + (((size_t)b * in_h + y) * in_w + x4) * 3;
    if (g.mode != 0) {
        for (int i = 0; i < 4; i++)
            letterbox_pixel(BgrSrc{frames + g.off, g.W}, g.H, g.W, o + 3 * i, x4 + i, y, g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2);
        return;
    }
    letterbox_pixels4(frames, (size_t)g.off, g.H, g.W, g.W, (unsigned *)o, x4, y, g.new_h, g.new_w, g.scale_x, g.scale_y, src_bytes);
}

// ---- tiled detection (fid_tile_cut): tile blockIdx.z of the table is cut from its frame into its own detector input ----
// A native tile (kind 0) is the rectangle copied to the top-left corner, the rest zero; a letterboxed one (kind 1) is letterbox_pixel /
// letterbox_pixels4 on the rectangle, whose rows are W pixels apart.  Only bytes of pixels inside the rectangle are read, except the
// guarded 4-byte fetch of letterbox_pixels4, which stays inside the frame batch.  The one-pixel form is letterbox_kernel over TileGeom.
__global__ void __launch_bounds__(256) tile_cut_kernel4_nv12(Nv12Batch nv, const fid::TileEntry *tab, uint8_t *out, int in_h, int in_w) {
    const int t = blockIdx.z;
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= in_w) return;
    const fid::TileEntry g = tab[t];
    letterbox_quad(nv.frame(g.frame, g.x0, g.y0).src, g.h, g.w, (unsigned *)(out + (((size_t)t * in_h + y) * in_w + x4) * 3), x4, y, g.new_h, g.new_w,
                   g.scale_x, g.scale_y, g.mode == 2);
}

// four output pixels per thread as three aligned dwords (in_w % 4 == 0), like letterbox_kernel4.  The branches are block-uniform.
__global__ void __launch_bounds__(256) tile_cut_kernel4(const uint8_t *frames, int H, int W, const fid::TileEntry *tab, uint8_t *out, int in_h, int in_w,
                                                        size_t src_bytes) {
    const int t = blockIdx.z;
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= in_w) return;
    const fid::TileEntry g = tab[t];
    const size_t fbase = (((size_t)g.frame * H + g.y0) * W + g.x0) * 3;
    uint8_t *o = out + (((size_t)t * in_h + y) * in_w + x4) * 3;
    if (g.kind == 0) {
        unsigned v[3] = {0u, 0u, 0u};
        if (y < g.h && x4 < g.w) {
            const uint8_t *q = frames + fbase + ((size_t)y * W + x4) * 3;     // (unaligned when W is odd or x0 is no multiple of 4)
            if (x4 + 4 <= g.w) {
                __builtin_memcpy(v, q, 12);                                    // the 12 bytes of four pixels inside the rectangle
            } else {
                const int nb = (g.w - x4) * 3;                                 // 3, 6 or 9 bytes: the row's last pixels, then zeros
                for (int k = 0; k < nb; k++) v[k >> 2] |= (unsigned)q[k] << (8 * (k & 3));
            }
        }
        unsigned *ow = (unsigned *)o;
        ow[0] = v[0]; ow[1] = v[1]; ow[2] = v[2];
        return;
    }
    if (g.mode != 0) {
        for (int i = 0; i < 4; i++)
            letterbox_pixel(BgrSrc{frames + fbase, W}, g.h, g.w, o + 3 * i, x4 + i, y, g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2);
        return;
    }
    letterbox_pixels4(frames, fbase, g.h, g.w, W, (unsigned *)o, x4, y, g.new_h, g.new_w, g.scale_x, g.scale_y, src_bytes);
}

// Host half of the mixed-size entry points: validate every image and compute its table entry (all-or-nothing: the caller enqueues nothing
// when this fails).  in_h = 0: no letterbox (the warp needs only the base pointer and H, W).
int ragged_entries(const int32_t *hw, const int64_t *offsets, size_t frames_bytes, int B, int in_h, int in_w, std::vector<fid::RaggedImg> &tab) {
    tab.resize(B);
    for (int b = 0; b < B; b++) {
        const int H = hw[2 * b], W = hw[2 * b + 1];
        FID_REQUIRE(H > 0 && W > 0, "image %d: bad size %dx%d", b, W, H);
        const unsigned long long bytes = (unsigned long long)H * (unsigned long long)W * 3ull;
        FID_REQUIRE(offsets[b] >= 0 && (unsigned long long)offsets[b] <= frames_bytes && bytes <= frames_bytes - (unsigned long long)offsets[b],
                    "image %d: bytes [%lld, %lld + %llu) leave the allocation of %zu bytes", b, (long long)offsets[b], (long long)offsets[b], bytes,
                    frames_bytes);
        fid::RaggedImg g{};
        if (in_h > 0) FID_REQUIRE(fid::ragged_geometry(H, W, in_h, in_w, &g), "image %d: degenerate letterbox %dx%d", b, g.new_w, g.new_h);
        else { g.H = H; g.W = W; }
        g.off = offsets[b];
        tab[b] = g;
    }
    return FID_OK;
}

// Host half of the NV12 entry points: validate the layout (all or nothing) and resolve the standard into the kernel argument.
int nv12_batch(const uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, Nv12Batch *nv) {
    const char *why = fid_nv12_check(desc, B, H, W);
    FID_REQUIRE(why == nullptr, "nv12: %s (B %d, %dx%d, pitch %d, uv_offset %lld, frame_stride %lld, standard %d)", why ? why : "", B, W, H,
                desc ? desc->pitch : 0, desc ? (long long)desc->uv_offset : 0ll, desc ? (long long)desc->frame_stride : 0ll,
                desc ? desc->standard : 0);
    nv->p = nv12; nv->frame_stride = desc->frame_stride; nv->uv_offset = desc->uv_offset; nv->pitch = desc->pitch;
    nv->H = H; nv->W = W;
    fid_yuv_coeffs_for(desc->standard, &nv->k);
    return FID_OK;
}

// The device table of a batch that has one (under the context's lock, before the launch): the host's n entries in, the device's out.
template <class Frames>
int upload_table(fid_ctx *, Frames &, int) { return FID_OK; }
int upload_table(fid_ctx *ctx, RaggedBatch &frames, int n) { return fid::ragged_table(ctx, frames.tab, n, &frames.tab); }

// Launch tail of the six fid_align_crops* entry points, which have validated every argument: n_rows crops from a batch of B frames.
template <class Frames, class Rows>
int launch_warp(fid_ctx *ctx, Frames frames, int B, Rows rows, int n_rows, const float *kps_dev, uint8_t *crops_dev, double *M_dev) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_TRY(upload_table(ctx, frames, B));
    hipLaunchKernelGGL((align_warp<Frames, Rows>), dim3(OUT / ROWS_PER_BLOCK, n_rows), dim3(256), 0, ctx->stream, frames, rows, kps_dev, crops_dev,
                       M_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// The four-pixel kernels write aligned dwords: whole quads per row, on an aligned output.
inline bool quads_fit(int in_w, const uint8_t *out_dev) { return in_w % 4 == 0 && ((size_t)out_dev & 3) == 0; }
inline dim3 quad_grid(int in_w, int in_h, int n) { return dim3(fid::cdiv(in_w / 4, 256), in_h, n); }

// The one-pixel letterbox kernel over n images (or tiles), enqueued by an entry point that holds the context's lock.
template <class Frames, class Geom>
void launch_letterbox(fid_ctx *ctx, const Frames &frames, const Geom &geom, int n, uint8_t *out_dev, int in_h, int in_w) {
    hipLaunchKernelGGL((letterbox_kernel<Frames, Geom>), dim3(fid::cdiv(in_w, 256), in_h, n), dim3(256), 0, ctx->stream, frames, geom, out_dev, in_h,
                       in_w);
}

}  // namespace

extern "C" {

int fid_align_crops(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, const float *kps_dev,
                    const int32_t *counts_dev, int cap, int faces_per_frame, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && frames_dev && kps_dev && counts_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && cap > 0 && faces_per_frame > 0, "bad sizes");
    FID_REQUIRE((long long)B * faces_per_frame <= 65535, "too many face slots per call (%lld)", (long long)B * faces_per_frame);
    return launch_warp(ctx, BgrBatch{frames_dev, H, W}, B, SlotRows{counts_dev, cap, faces_per_frame}, B * faces_per_frame, kps_dev, crops_dev, M_dev);
}

int fid_align_crops_packed(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, const float *kps_dev, int cap,
                           const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && frames_dev && kps_dev && src_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && cap > 0 && n_rows > 0, "bad sizes");
    FID_REQUIRE((long long)B * cap <= 0x7FFFFFFFll, "B * cap = %lld overflows the row table's int32 entries", (long long)B * cap);
    FID_REQUIRE(n_rows <= 65535, "too many face rows per call (%d)", n_rows);
    return launch_warp(ctx, BgrBatch{frames_dev, H, W}, B, PackedRows{src_dev, B, cap}, n_rows, kps_dev, crops_dev, M_dev);
}

int fid_letterbox(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, uint8_t *out_dev, int in_h, int in_w,
                  double *det_scale) {
    FID_REQUIRE(ctx && frames_dev && out_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && in_h > 0 && in_w > 0 && B <= 65535 && in_h <= 65535, "bad sizes");
    fid::RaggedImg g{};
    FID_REQUIRE(fid::ragged_geometry(H, W, in_h, in_w, &g), "degenerate letterbox %dx%d", g.new_w, g.new_h);
    if (det_scale) *det_scale = (double)g.new_h / (double)H;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    if (g.mode == 0 && quads_fit(in_w, out_dev))
        hipLaunchKernelGGL(letterbox_kernel4, quad_grid(in_w, in_h, B), dim3(256), 0, ctx->stream, frames_dev, H, W, out_dev, in_h, in_w, g.new_h,
                           g.new_w, g.scale_x, g.scale_y, (size_t)B * H * W * 3);
    else
        launch_letterbox(ctx, BgrBatch{frames_dev, H, W}, UniformGeom{g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2}, B, out_dev, in_h, in_w);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// ---- tiled detection: T rectangles of the frames, each cut into its own detector input (tiles: host [T,6], include/faceid.h) ----
int fid_tile_cut(fid_ctx *ctx, const uint8_t *frames_dev, int B, int H, int W, const int32_t *tiles, int T, uint8_t *out_dev, int in_h, int in_w) {
    FID_REQUIRE(ctx && frames_dev && tiles && out_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && in_h > 0 && in_w > 0 && T > 0 && T <= 65535 && in_h <= 65535, "bad sizes");
    std::vector<fid::TileEntry> host;
    FID_TRY(fid::tile_entries(tiles, T, B, H, W, in_h, in_w, host, nullptr));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    const fid::TileEntry *tab;
    FID_TRY(fid::tile_table(ctx, host.data(), T, &tab));
    if (quads_fit(in_w, out_dev))
        hipLaunchKernelGGL(tile_cut_kernel4, quad_grid(in_w, in_h, T), dim3(256), 0, ctx->stream, frames_dev, H, W, tab, out_dev, in_h, in_w,
                           (size_t)B * H * W * 3);
    else
        launch_letterbox(ctx, BgrBatch{frames_dev, H, W}, TileGeom{tab}, T, out_dev, in_h, in_w);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// ---- mixed-size batches: image b is dense uint8 [H_b, W_b, 3] at frames_dev + offsets[b] (the reference runs all of these per image) ----
int fid_letterbox_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets, int B,
                         uint8_t *out_dev, int in_h, int in_w, double *det_scale) {
    FID_REQUIRE(ctx && frames_dev && hw && offsets && out_dev, "NULL argument");
    FID_REQUIRE(B > 0 && in_h > 0 && in_w > 0 && B <= 65535 && in_h <= 65535, "bad sizes");
    std::vector<fid::RaggedImg> host;
    FID_TRY(ragged_entries(hw, offsets, frames_bytes, B, in_h, in_w, host));
    if (det_scale)
        for (int b = 0; b < B; b++) det_scale[b] = (double)host[b].new_h / (double)host[b].H;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    RaggedBatch frames{frames_dev, host.data()};
    FID_TRY(upload_table(ctx, frames, B));
    if (quads_fit(in_w, out_dev))
        hipLaunchKernelGGL(letterbox_kernel4_ragged, quad_grid(in_w, in_h, B), dim3(256), 0, ctx->stream, frames_dev, frames.tab, out_dev, in_h, in_w,
                           frames_bytes);
    else
        launch_letterbox(ctx, frames, RaggedGeom{}, B, out_dev, in_h, in_w);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_align_crops_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets, int B,
                           const float *kps_dev, const int32_t *counts_dev, int cap, int faces_per_frame, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && frames_dev && hw && offsets && kps_dev && counts_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && cap > 0 && faces_per_frame > 0, "bad sizes");
    FID_REQUIRE((long long)B * faces_per_frame <= 65535, "too many face slots per call (%lld)", (long long)B * faces_per_frame);
    std::vector<fid::RaggedImg> host;
    FID_TRY(ragged_entries(hw, offsets, frames_bytes, B, 0, 0, host));
    return launch_warp(ctx, RaggedBatch{frames_dev, host.data()}, B, SlotRows{counts_dev, cap, faces_per_frame}, B * faces_per_frame, kps_dev,
                       crops_dev, M_dev);
}

int fid_align_crops_packed_ragged(fid_ctx *ctx, const uint8_t *frames_dev, size_t frames_bytes, const int32_t *hw, const int64_t *offsets, int B,
                                  const float *kps_dev, int cap, const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && frames_dev && hw && offsets && kps_dev && src_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && cap > 0 && n_rows > 0, "bad sizes");
    FID_REQUIRE((long long)B * cap <= 0x7FFFFFFFll, "B * cap = %lld overflows the row table's int32 entries", (long long)B * cap);
    FID_REQUIRE(n_rows <= 65535, "too many face rows per call (%d)", n_rows);
    std::vector<fid::RaggedImg> host;
    FID_TRY(ragged_entries(hw, offsets, frames_bytes, B, 0, 0, host));
    return launch_warp(ctx, RaggedBatch{frames_dev, host.data()}, B, PackedRows{src_dev, B, cap}, n_rows, kps_dev, crops_dev, M_dev);
}

// ---- NV12 frames (include/faceid.h): the conversion alone, both ways, and the four frame readers with the conversion fused into their taps ----
int fid_nv12_to_bgr_host(const uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, uint8_t *bgr_out) {
    FID_REQUIRE(nv12 && bgr_out, "NULL argument");
    const char *why = fid_nv12_check(desc, B, H, W);
    FID_REQUIRE(why == nullptr, "nv12: %s", why ? why : "");
    fid_nv12_to_bgr_frames_host(nv12, desc, B, H, W, bgr_out);
    return FID_OK;
}

int fid_nv12_to_bgr(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, uint8_t *bgr_out_dev) {
    FID_REQUIRE(ctx && nv12_dev && bgr_out_dev, "NULL argument");
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_dev, desc, B, H, W, &nv));
    FID_REQUIRE(B <= 65535 && H <= 65535, "bad sizes");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    dim3 grid(fid::cdiv(W / 2, 256), H, B);
    hipLaunchKernelGGL(nv12_to_bgr_kernel, grid, dim3(256), 0, ctx->stream, nv, bgr_out_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_bgr_to_nv12_host(const uint8_t *bgr, int B, int H, int W, uint8_t *nv12_out, const fid_nv12_desc *desc) {
    FID_REQUIRE(bgr && nv12_out, "NULL argument");
    const char *why = fid_nv12_check(desc, B, H, W);
    FID_REQUIRE(why == nullptr, "nv12: %s", why ? why : "");
    fid_bgr_to_nv12_frames_host(bgr, B, H, W, nv12_out, desc);
    return FID_OK;
}

int fid_bgr_to_nv12(fid_ctx *ctx, const uint8_t *bgr_dev, int B, int H, int W, uint8_t *nv12_out_dev, const fid_nv12_desc *desc) {
    FID_REQUIRE(ctx && bgr_dev && nv12_out_dev, "NULL argument");
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_out_dev, desc, B, H, W, &nv));
    FID_REQUIRE(B <= 65535, "bad sizes");
    const uintptr_t in0 = (uintptr_t)bgr_dev, in1 = in0 + (size_t)B * H * W * 3, out0 = (uintptr_t)nv12_out_dev;
    const uintptr_t out1 = out0 + (size_t)(B - 1) * (size_t)desc->frame_stride + (size_t)desc->uv_offset + (size_t)desc->pitch * (H / 2);
    FID_REQUIRE(in1 <= out0 || out1 <= in0, "bgr_to_nv12: the BGR frames and the NV12 frames overlap");
    const int quads = fid::cdiv(W, 4);
    const long long per_frame = (long long)quads * (H / 2);
    FID_REQUIRE(per_frame <= 0x7FFFFFFFll - 256, "bad sizes");
    Nv12Out o{nv12_out_dev, desc->frame_stride, desc->uv_offset, desc->pitch, {}};
    fid_yuv_fwd_for(desc->standard, &o.k);
    const int wide = W % 4 == 0 && in0 % 4 == 0 && out0 % 4 == 0 && desc->pitch % 4 == 0 && desc->uv_offset % 4 == 0 && desc->frame_stride % 4 == 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    dim3 grid((unsigned)fid::cdiv64(per_frame, 256), B);
    hipLaunchKernelGGL(bgr_to_nv12_kernel, grid, dim3(256), 0, ctx->stream, bgr_dev, H, W, quads, (int)per_frame, o, wide);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_letterbox_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, uint8_t *out_dev, int in_h,
                       int in_w, double *det_scale) {
    FID_REQUIRE(ctx && nv12_dev && out_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && in_h > 0 && in_w > 0 && B <= 65535 && in_h <= 65535, "bad sizes");
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_dev, desc, B, H, W, &nv));
    fid::RaggedImg g{};
    FID_REQUIRE(fid::ragged_geometry(H, W, in_h, in_w, &g), "degenerate letterbox %dx%d", g.new_w, g.new_h);
    if (det_scale) *det_scale = (double)g.new_h / (double)H;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // (one output pixel per thread: with four, 32 frames of 1080p -> 640x640 took 0.053 instead of 0.048 ms -- docs/FINDINGS.md)
    launch_letterbox(ctx, nv, UniformGeom{g.new_h, g.new_w, g.scale_x, g.scale_y, g.mode == 2}, B, out_dev, in_h, in_w);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_tile_cut_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const int32_t *tiles, int T,
                      uint8_t *out_dev, int in_h, int in_w) {
    FID_REQUIRE(ctx && nv12_dev && tiles && out_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && in_h > 0 && in_w > 0 && T > 0 && T <= 65535 && in_h <= 65535, "bad sizes");
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_dev, desc, B, H, W, &nv));
    std::vector<fid::TileEntry> host;
    FID_TRY(fid::tile_entries(tiles, T, B, H, W, in_h, in_w, host, nullptr));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    const fid::TileEntry *tab;
    FID_TRY(fid::tile_table(ctx, host.data(), T, &tab));
    if (quads_fit(in_w, out_dev))
        hipLaunchKernelGGL(tile_cut_kernel4_nv12, quad_grid(in_w, in_h, T), dim3(256), 0, ctx->stream, nv, tab, out_dev, in_h, in_w);
    else
        launch_letterbox(ctx, nv, TileGeom{tab}, T, out_dev, in_h, in_w);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_align_crops_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *kps_dev,
                         const int32_t *counts_dev, int cap, int faces_per_frame, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && nv12_dev && kps_dev && counts_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && cap > 0 && faces_per_frame > 0, "bad sizes");
    FID_REQUIRE((long long)B * faces_per_frame <= 65535, "too many face slots per call (%lld)", (long long)B * faces_per_frame);
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_dev, desc, B, H, W, &nv));
    return launch_warp(ctx, nv, B, SlotRows{counts_dev, cap, faces_per_frame}, B * faces_per_frame, kps_dev, crops_dev, M_dev);
}

int fid_align_crops_packed_nv12(fid_ctx *ctx, const uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *kps_dev,
                                int cap, const int32_t *src_dev, int n_rows, uint8_t *crops_dev, double *M_dev) {
    FID_REQUIRE(ctx && nv12_dev && kps_dev && src_dev && crops_dev, "NULL argument");
    FID_REQUIRE(B > 0 && H > 0 && W > 0 && cap > 0 && n_rows > 0, "bad sizes");
    FID_REQUIRE((long long)B * cap <= 0x7FFFFFFFll, "B * cap = %lld overflows the row table's int32 entries", (long long)B * cap);
    FID_REQUIRE(n_rows <= 65535, "too many face rows per call (%d)", n_rows);
    Nv12Batch nv;
    FID_TRY(nv12_batch(nv12_dev, desc, B, H, W, &nv));
    return launch_warp(ctx, nv, B, PackedRows{src_dev, B, cap}, n_rows, kps_dev, crops_dev, M_dev);
}

}  // extern "C"
