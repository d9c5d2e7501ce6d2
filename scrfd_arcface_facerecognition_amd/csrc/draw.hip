// Drawing detections, names and scores onto frames, on the device: the fourth step of the reference's demo loop (main.py:130-148 with
// utils/helpers.py:126-179), enqueued behind the match with nothing read back first.  The arithmetic -- face record, label text, pixel
// coverage -- is draw_core.h's, shared with the host rasteriser fid_draw_faces_host below.
//
// A gather, not a scatter: where two faces' overlays overlap the LATER face shows (the reference draws them one after another), and one
// workgroup per face painting its own primitives would leave that to the scheduler.  Two kernels per call, ordered by the stream:
//
//   draw_prepare   one thread per (frame, face slot): the face record into a [B, cap] table in the context's scratch, its clipped extent into
//                  a table of its own (16 bytes per face: what the cull reads), and the frame's face count.
//   draw_paint     256 threads per 64 x 16-pixel tile.  Cull: each thread tests one extent against the tile; ballot + prefix popcount, with the
//                  per-wave counts in LDS, list the tile's faces in ascending order (256 at a time when a frame has more).  A tile that
//                  lies inside a box's empty interior, off its bar and its text, is not that face's (fid_draw_touches).  A tile no face
//                  touches -- most tiles -- ends there.  Paint: the listed records (and the font, if one has text) go to LDS; each thread owns
//                  four adjacent pixels of one row, walks the list in order and keeps the colour of the last face that covers each.  Store:
//                  nothing is read from the frame; four covered pixels in a frame whose rows are dword-aligned are three dword stores,
//                  anything else byte stores of the covered pixels only.
//
// NV12 frames (fid_draw_faces_nv12): draw_prepare as it is, then draw_paint_nv12 -- draw_paint's tiles, cull and walk, with each pixel also
// keeping the INDEX of its last covering face.  Y: the pixel's own last face.  A chroma pair belongs to the last face that covers any of the
// four pixels of its group, and the listed faces ascend, over the cull passes and the record chunks too: that face is the maximum of the four
// indices.  Rows 2k and 2k+1 of a tile are 16 lanes apart in one wave, so a thread reduces its own two pixels per group and exchanges the
// result with lane ^ 16; the even row stores the pairs.  Four covered Y bytes, or two written pairs, are one dword in a layout of dwords.
//
// This file must never get a fast-math flag: bar height and label digits are compared bit for bit with the host's.
#include <cmath>
#include <vector>

#include "common.h"
#include "draw_core.h"
#include "draw_nv12_core.h"

struct fid_labels {
    int G = 0, device = 0;
    fid_draw_label *dev = nullptr;           // [G]
};

namespace {

using fid::cdiv;

const uint8_t h_font[FID_DRAW_GLYPHS * 7] = FID_DRAW_FONT_INIT;
__device__ const uint8_t d_font[FID_DRAW_GLYPHS * 7] = FID_DRAW_FONT_INIT;

constexpr int TILE_W = 64, TILE_H = 16;
constexpr int MAX_GRID = 1 << 18;
constexpr int REC_CHUNK = 64;               // records in LDS at a time: 6.4 KB, so that LDS does not bound the waves per CU

struct PrepArgs {
    const float *det;
    const int32_t *counts, *idx;
    const float *score;
    const int32_t *offsets, *track;
    const fid_draw_label *labels;
    int G, B, cap, id_stride, n_rows, H, W;
    fid_draw_style st;
    int32_t *nb;                             // [B] faces of frame b
    int4 *ext;                               // [B, cap] clipped extents (x0, y0, x1, y1), x0 > x1: nothing
    fid_draw_face *rec;                      // [B, cap]
};

__global__ void __launch_bounds__(256) draw_prepare(const PrepArgs a) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)a.B * a.cap) return;
    const int b = (int)(gid / a.cap), f = (int)(gid % a.cap);
    int row0;
    const int n = fid_draw_face_count(b, a.counts, a.cap, a.idx != nullptr, a.id_stride, a.offsets, a.n_rows, &row0);
    if (f == 0) a.nb[b] = n;
    int4 e = make_int4(1, 1, 0, 0);
    if (f < n) {
        int ii = -1;
        float sc = 0.f;
        if (a.idx) {
            const long long i = a.offsets ? (long long)row0 + f : (long long)b * a.id_stride + f;
            ii = a.idx[i]; sc = a.score[i];
        }
        const bool known = a.labels != nullptr && ii >= 0 && ii < a.G;
        const int tid = a.track ? a.track[gid * 2] : -1;
        fid_draw_face fc;
        fid_draw_make_face(&fc, a.det + gid * 5, known ? a.labels + ii : nullptr, sc, tid, &a.st, a.H, a.W);
        e = make_int4(fc.ex0, fc.ey0, fc.ex1, fc.ey1);
        if (e.x <= e.z) a.rec[gid] = fc;
    }
    a.ext[gid] = e;
}

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__global__ void __launch_bounds__(256) draw_paint(uint8_t *__restrict__ frames, const int32_t *__restrict__ nb, const int4 *__restrict__ ext,
                                                  const uint32_t *__restrict__ rec, int H, int W, int cap, int ntx, int tiles_per_frame,
                                                  long long total_tiles, int r, int t, int dword_rows) {
    __shared__ uint32_t s_rec[REC_CHUNK * FID_DRAW_FACE_WORDS];
    __shared__ int s_list[256];
    __shared__ int s_wcount[4];
    __shared__ uint8_t s_font[FID_DRAW_GLYPHS * 7 + 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool font_loaded = false;                // (block-uniform)
    for (long long tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_frame), rem = (int)(tile % tiles_per_frame);
        const int X0 = (rem % ntx) * TILE_W, Y0 = (rem / ntx) * TILE_H;
        const int X1 = min(X0 + TILE_W - 1, W - 1), Y1 = min(Y0 + TILE_H - 1, H - 1);
        const int px = X0 + (tid & 15) * 4, py = Y0 + (tid >> 4);
        const int n = nb[b];
        uint32_t col[4] = {0u, 0u, 0u, 0u};
        unsigned cov = 0u;
        for (int f0 = 0; f0 < n; f0 += 256) {
            const int f = f0 + tid;
            bool hit = false;
            if (f < n) {
                const int4 e = ext[(size_t)b * cap + f];
                hit = e.x <= e.z && e.x <= X1 && e.z >= X0 && e.y <= Y1 && e.w >= Y0;
                // the extent holds the box's empty interior: a tile inside it, off the bar and off the text, is none of this face's
                if (hit) hit = fid_draw_touches((const fid_draw_face *)(rec + ((size_t)b * cap + f) * FID_DRAW_FACE_WORDS), X0, Y0, X1, Y1, r, t);
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) s_wcount[wave] = __popcll(m);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int c = s_wcount[w];
                base += w < wave ? c : 0;
                total += c;
            }
            if (hit) s_list[base + lanes_below(m, lane)] = f;
            __syncthreads();
            if (total == 0) continue;        // (block-uniform: nothing of this chunk touches the tile)
            for (int j0 = 0; j0 < total; j0 += REC_CHUNK) {             // the listed records through LDS, REC_CHUNK at a time, in list order
                const int nrec = min(REC_CHUNK, total - j0);
                for (int i = tid; i < nrec * FID_DRAW_FACE_WORDS; i += 256) {
                    const int j = i / FID_DRAW_FACE_WORDS, k = i - j * FID_DRAW_FACE_WORDS;
                    s_rec[i] = rec[((size_t)b * cap + s_list[j0 + j]) * FID_DRAW_FACE_WORDS + k];
                }
                const bool my_text = tid < nrec && (rec[((size_t)b * cap + s_list[j0 + (tid < nrec ? tid : 0)]) * FID_DRAW_FACE_WORDS + 11] & 0xFFu) != 0u;
                const int any_text = __syncthreads_or(my_text);
                if (any_text && !font_loaded) {
                    for (int i = tid; i < FID_DRAW_GLYPHS * 7; i += 256) s_font[i] = d_font[i];
                    font_loaded = true;
                    __syncthreads();
                }
                if (py <= Y1) {
                    for (int j = 0; j < nrec; j++) {
                        const fid_draw_face *fc = (const fid_draw_face *)(s_rec + j * FID_DRAW_FACE_WORDS);
                        if (!fid_draw_touches(fc, px, py, px + 3, py, r, t)) continue;
                        const uint32_t c = (uint32_t)fc->bgr[0] | ((uint32_t)fc->bgr[1] << 8) | ((uint32_t)fc->bgr[2] << 16);
#pragma unroll
                        for (int p = 0; p < 4; p++)
                            if (fid_draw_covers(fc, px + p, py, r, t, s_font)) { col[p] = c; cov |= 1u << p; }
                    }
                }
                __syncthreads();             // the next chunk, pass or tile rewrites s_rec / s_list
            }
        }
        if (cov != 0u) {                     // (a covered pixel lies inside the frame: extents are clipped to it)
            uint8_t *dst = frames + (((size_t)b * H + py) * W + px) * 3;
            if (cov == 15u && dword_rows) {
                uint32_t *d = (uint32_t *)dst;
                d[0] = col[0] | (col[1] << 24);
                d[1] = (col[1] >> 8) | (col[2] << 16);
                d[2] = (col[2] >> 16) | (col[3] << 8);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (cov & (1u << p)) {
                        dst[p * 3] = (uint8_t)col[p]; dst[p * 3 + 1] = (uint8_t)(col[p] >> 8); dst[p * 3 + 2] = (uint8_t)(col[p] >> 16);
                    }
            }
        }
    }
}

// the layout of the NV12 frames a kernel draws on (fid_nv12_desc with the standard's forward integers resolved on the host)
struct Nv12Target {
    uint8_t *p;
    long long frame_stride, uv_offset;
    int pitch, y_dwords, uv_dwords;
    fid_yuv_fwd k;
};

// draw_paint on two planes.  The tile, the cull and the walk are draw_paint's, kept apart so that the BGR kernel stays as it is.
__global__ void __launch_bounds__(256) draw_paint_nv12(const Nv12Target o, const int32_t *__restrict__ nb, const int4 *__restrict__ ext,
                                                       const uint32_t *__restrict__ rec, int H, int W, int cap, int ntx, int tiles_per_frame,
                                                       long long total_tiles, int r, int t) {
    __shared__ uint32_t s_rec[REC_CHUNK * FID_DRAW_FACE_WORDS];
    __shared__ int s_list[256];
    __shared__ int s_wcount[4];
    __shared__ uint8_t s_font[FID_DRAW_GLYPHS * 7 + 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool font_loaded = false;                // (block-uniform)
    for (long long tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_frame), rem = (int)(tile % tiles_per_frame);
        const int X0 = (rem % ntx) * TILE_W, Y0 = (rem / ntx) * TILE_H;
        const int X1 = min(X0 + TILE_W - 1, W - 1), Y1 = min(Y0 + TILE_H - 1, H - 1);
        const int px = X0 + (tid & 15) * 4, py = Y0 + (tid >> 4);
        const int n = nb[b];
        uint32_t col[4] = {0u, 0u, 0u, 0u};
        int last[4] = {-1, -1, -1, -1};      // the face whose colour col[p] is; -1: not covered
        bool touched = false;                // (block-uniform)
        for (int f0 = 0; f0 < n; f0 += 256) {
            const int f = f0 + tid;
            bool hit = false;
            if (f < n) {
                const int4 e = ext[(size_t)b * cap + f];
                hit = e.x <= e.z && e.x <= X1 && e.z >= X0 && e.y <= Y1 && e.w >= Y0;
                if (hit) hit = fid_draw_touches((const fid_draw_face *)(rec + ((size_t)b * cap + f) * FID_DRAW_FACE_WORDS), X0, Y0, X1, Y1, r, t);
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) s_wcount[wave] = __popcll(m);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int c = s_wcount[w];
                base += w < wave ? c : 0;
                total += c;
            }
            if (hit) s_list[base + lanes_below(m, lane)] = f;
            __syncthreads();
            if (total == 0) continue;        // (block-uniform: nothing of this chunk touches the tile)
            touched = true;
            for (int j0 = 0; j0 < total; j0 += REC_CHUNK) {
                const int nrec = min(REC_CHUNK, total - j0);
                for (int i = tid; i < nrec * FID_DRAW_FACE_WORDS; i += 256) {
                    const int j = i / FID_DRAW_FACE_WORDS, k = i - j * FID_DRAW_FACE_WORDS;
                    s_rec[i] = rec[((size_t)b * cap + s_list[j0 + j]) * FID_DRAW_FACE_WORDS + k];
                }
                const bool my_text = tid < nrec && (rec[((size_t)b * cap + s_list[j0 + (tid < nrec ? tid : 0)]) * FID_DRAW_FACE_WORDS + 11] & 0xFFu) != 0u;
                const int any_text = __syncthreads_or(my_text);
                if (any_text && !font_loaded) {
                    for (int i = tid; i < FID_DRAW_GLYPHS * 7; i += 256) s_font[i] = d_font[i];
                    font_loaded = true;
                    __syncthreads();
                }
                if (py <= Y1) {
                    for (int j = 0; j < nrec; j++) {
                        const fid_draw_face *fc = (const fid_draw_face *)(s_rec + j * FID_DRAW_FACE_WORDS);
                        if (!fid_draw_touches(fc, px, py, px + 3, py, r, t)) continue;
                        const uint32_t c = (uint32_t)fc->bgr[0] | ((uint32_t)fc->bgr[1] << 8) | ((uint32_t)fc->bgr[2] << 16);
                        const int fi = s_list[j0 + j];
#pragma unroll
                        for (int p = 0; p < 4; p++)
                            if (fid_draw_covers(fc, px + p, py, r, t, s_font)) { col[p] = c; last[p] = fi; }
                    }
                }
                __syncthreads();             // the next chunk, pass or tile rewrites s_rec / s_list
            }
        }
        if (!touched) continue;              // a tile no face touches -- most tiles -- ends here
        // chroma: per group the face of the highest index over its four pixels -- this row's two, and the other row's from lane ^ 16.  Every
        // lane takes part in the exchange (a row below the frame holds -1; H is even, so a group's two rows are in the frame or out together)
        int gl[2];
        uint32_t gc[2];
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const bool second = last[2 * g + 1] > last[2 * g];
            gl[g] = second ? last[2 * g + 1] : last[2 * g];
            gc[g] = second ? col[2 * g + 1] : col[2 * g];
            const int ol = __shfl_xor(gl[g], 16);
            const uint32_t oc = (uint32_t)__shfl_xor((int)gc[g], 16);
            if (ol > gl[g]) { gl[g] = ol; gc[g] = oc; }
        }
        uint8_t *frame = o.p + (size_t)b * (size_t)o.frame_stride;
        const unsigned cov = (last[0] >= 0 ? 1u : 0u) | (last[1] >= 0 ? 2u : 0u) | (last[2] >= 0 ? 4u : 0u) | (last[3] >= 0 ? 8u : 0u);
        if (cov != 0u) {                     // (a covered pixel lies inside the frame: extents are clipped to it)
            uint8_t *dst = frame + (size_t)py * o.pitch + px;
            uint32_t yv = 0u;
#pragma unroll
            for (int p = 0; p < 4; p++)
                yv |= (uint32_t)fid_yuv_luma(o.k, (int)(col[p] & 255u), (int)((col[p] >> 8) & 255u), (int)((col[p] >> 16) & 255u)) << (8 * p);
            if (cov == 15u && o.y_dwords) {
                *(uint32_t *)dst = yv;
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (cov & (1u << p)) dst[p] = (uint8_t)(yv >> (8 * p));
            }
        }
        if (((tid >> 4) & 1) == 0 && (gl[0] >= 0 || gl[1] >= 0)) {       // the even row of each pair of rows stores the group's pair
            uint8_t *dst = frame + (size_t)o.uv_offset + (size_t)(py >> 1) * o.pitch + px;
            uint32_t uvv = 0u;
#pragma unroll
            for (int g = 0; g < 2; g++) {
                int uv[2];
                fid_yuv_chroma(o.k, 4 * (int)(gc[g] & 255u), 4 * (int)((gc[g] >> 8) & 255u), 4 * (int)((gc[g] >> 16) & 255u), uv);
                uvv |= ((uint32_t)uv[0] | ((uint32_t)uv[1] << 8)) << (16 * g);
            }
            if (gl[0] >= 0 && gl[1] >= 0 && o.uv_dwords) {
                *(uint32_t *)dst = uvv;
            } else {
#pragma unroll
                for (int g = 0; g < 2; g++)
                    if (gl[g] >= 0) { dst[2 * g] = (uint8_t)(uvv >> (16 * g)); dst[2 * g + 1] = (uint8_t)(uvv >> (16 * g + 8)); }
            }
        }
    }
}

int check_draw(const void *frames, int B, int H, int W, const void *det, const void *counts, int cap, const void *idx, const void *score,
               int id_stride, const void *offsets, int n_rows, const fid_draw_style *st) {
    const char *why = fid_draw_check(frames, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, st);
    FID_REQUIRE(why == nullptr, "draw: %s", why ? why : "");
    return FID_OK;
}

int check_nv12(const fid_nv12_desc *desc, int B, int H, int W) {
    const char *why = fid_nv12_check(desc, B, H, W);
    FID_REQUIRE(why == nullptr, "draw: nv12: %s", why ? why : "");
    return FID_OK;
}

// the caller's names / name_offsets / bgr as G label rows
int make_labels(const char *names, const int32_t *name_offsets, const uint8_t *bgr, int G, std::vector<fid_draw_label> &tab) {
    FID_REQUIRE(G > 0 && name_offsets, "labels: G %d must be positive and name_offsets given", G);
    FID_REQUIRE(name_offsets[0] >= 0, "labels: name_offsets[0] = %d is negative", name_offsets[0]);
    for (int g = 0; g < G; g++)
        FID_REQUIRE(name_offsets[g + 1] >= name_offsets[g], "labels: name_offsets[%d] = %d below name_offsets[%d] = %d", g + 1, name_offsets[g + 1], g,
                    name_offsets[g]);
    FID_REQUIRE(names || name_offsets[G] == name_offsets[0], "labels: NULL names");
    tab.resize(G);
    for (int g = 0; g < G; g++)
        fid_draw_make_label(&tab[g], g, names ? names + name_offsets[g] : nullptr, name_offsets[g + 1] - name_offsets[g], bgr ? bgr + 3 * (size_t)g : nullptr);
    return FID_OK;
}

// the first kernel of a draw call, BGR or NV12: the face tables in the context's scratch (the context's lock is held, its device is set)
int prepare_faces(fid_ctx *ctx, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap, const int32_t *idx_dev,
                  const float *score_dev, int id_stride, const int32_t *offsets_dev, int n_rows, const int32_t *track_dev, fid_labels *labels,
                  const fid_draw_style *style, PrepArgs *out) {
    const size_t faces = (size_t)B * cap;
    const size_t off_ext = ((size_t)B * 4 + 15) & ~(size_t)15, off_rec = off_ext + faces * sizeof(int4);
    void *ws;
    FID_TRY(fid::get_scratch(ctx, 2, off_rec + faces * sizeof(fid_draw_face), &ws));
    PrepArgs a{};
    a.det = det_dev; a.counts = counts_dev; a.idx = idx_dev; a.score = score_dev;
    a.offsets = idx_dev ? offsets_dev : nullptr; a.track = track_dev;
    a.labels = labels ? labels->dev : nullptr; a.G = labels ? labels->G : 0;
    a.B = B; a.cap = cap; a.id_stride = id_stride; a.n_rows = n_rows; a.H = H; a.W = W;
    a.st = *style;
    a.nb = (int32_t *)ws; a.ext = (int4 *)((char *)ws + off_ext); a.rec = (fid_draw_face *)((char *)ws + off_rec);
    hipLaunchKernelGGL(draw_prepare, dim3((unsigned)fid::cdiv64((int64_t)faces, 256)), dim3(256), 0, ctx->stream, a);
    *out = a;
    return FID_OK;
}

}  // namespace

extern "C" {

int fid_labels_create(fid_ctx *ctx, const char *names, const int32_t *name_offsets, const uint8_t *bgr, int G, fid_labels **out) {
    FID_REQUIRE(ctx && out, "labels: NULL argument");
    std::vector<fid_draw_label> tab;
    FID_TRY(make_labels(names, name_offsets, bgr, G, tab));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    fid_labels *l = new fid_labels();
    l->G = G; l->device = ctx->device;
    if (hipMalloc((void **)&l->dev, (size_t)G * sizeof(fid_draw_label)) != hipSuccess) {
        delete l;
        fid::set_error("labels: out of device memory for %d rows", G);
        return FID_E_NOMEM;
    }
    if (hipMemcpy(l->dev, tab.data(), (size_t)G * sizeof(fid_draw_label), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(l->dev);
        delete l;
        fid::set_error("labels: the copy of %d rows to the device failed", G);
        return FID_E_HIP;
    }
    *out = l;
    return FID_OK;
}

int fid_labels_destroy(fid_ctx *ctx, fid_labels *labels) {
    FID_REQUIRE(ctx, "labels: NULL context");
    if (!labels) return FID_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    if (labels->dev) (void)hipFree(labels->dev);
    delete labels;
    return FID_OK;
}

int fid_draw_faces(fid_ctx *ctx, uint8_t *frames_dev, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap,
                   const int32_t *idx_dev, const float *score_dev, int id_stride, const int32_t *offsets_dev, int n_rows,
                   const int32_t *track_dev, fid_labels *labels, const fid_draw_style *style) {
    FID_REQUIRE(ctx, "draw: NULL context");
    FID_TRY(check_draw(frames_dev, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, style));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    PrepArgs a{};
    FID_TRY(prepare_faces(ctx, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, track_dev, labels, style, &a));
    const int ntx = cdiv(W, TILE_W), nty = cdiv(H, TILE_H);
    const long long tiles_per_frame = (long long)ntx * nty, total = tiles_per_frame * B;      // (H * W * 3 fits int32: so does ntx * nty)
    const int grid = (int)std::min<long long>(total, MAX_GRID);
    const int dword_rows = (W % 4 == 0) && ((uintptr_t)frames_dev % 4 == 0);
    hipLaunchKernelGGL(draw_paint, dim3(grid), dim3(256), 0, ctx->stream, frames_dev, (const int32_t *)a.nb, (const int4 *)a.ext,
                       (const uint32_t *)a.rec, H, W, cap, ntx, (int)tiles_per_frame, total, (style->thickness - 1) / 2, style->text_scale,
                       dword_rows);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_draw_faces_host(uint8_t *frames, int B, int H, int W, const float *det, const int32_t *counts, int cap, const int32_t *idx,
                        const float *score, int id_stride, const int32_t *offsets, int n_rows, const int32_t *track, const char *names,
                        const int32_t *name_offsets, const uint8_t *bgr, int G, const fid_draw_style *style) {
    FID_TRY(check_draw(frames, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, style));
    std::vector<fid_draw_label> tab;
    if (name_offsets) FID_TRY(make_labels(names, name_offsets, bgr, G, tab));
    const int nG = (int)tab.size(), r = (style->thickness - 1) / 2, t = style->text_scale;
    if (!idx) offsets = nullptr;
    for (int b = 0; b < B; b++) {
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, idx != nullptr, id_stride, offsets, n_rows, &row0);
        uint8_t *img = frames + (size_t)b * H * W * 3;
        for (int f = 0; f < n; f++) {          // ascending: a later face overwrites an earlier one
            const size_t slot = (size_t)b * cap + f;
            int ii = -1;
            float sc = 0.f;
            if (idx) {
                const size_t i = offsets ? (size_t)row0 + f : (size_t)b * id_stride + f;
                ii = idx[i]; sc = score[i];
            }
            const bool known = ii >= 0 && ii < nG;
            fid_draw_face fc;
            fid_draw_make_face(&fc, det + slot * 5, known ? &tab[ii] : nullptr, sc, track ? track[slot * 2] : -1, style, H, W);
            for (int y = fc.ey0; y <= fc.ey1; y++)
                for (int x = fc.ex0; x <= fc.ex1; x++)
                    if (fid_draw_covers(&fc, x, y, r, t, h_font)) {
                        uint8_t *p = img + ((size_t)y * W + x) * 3;
                        p[0] = fc.bgr[0]; p[1] = fc.bgr[1]; p[2] = fc.bgr[2];
                    }
        }
    }
    return FID_OK;
}

int fid_draw_faces_nv12(fid_ctx *ctx, uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *det_dev,
                        const int32_t *counts_dev, int cap, const int32_t *idx_dev, const float *score_dev, int id_stride,
                        const int32_t *offsets_dev, int n_rows, const int32_t *track_dev, fid_labels *labels, const fid_draw_style *style) {
    FID_REQUIRE(ctx, "draw: NULL context");
    FID_TRY(check_draw(nv12_dev, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, style));
    FID_TRY(check_nv12(desc, B, H, W));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    PrepArgs a{};
    FID_TRY(prepare_faces(ctx, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, track_dev, labels, style, &a));
    const int ntx = cdiv(W, TILE_W), nty = cdiv(H, TILE_H);
    const long long tiles_per_frame = (long long)ntx * nty, total = tiles_per_frame * B;
    const int grid = (int)std::min<long long>(total, MAX_GRID);
    Nv12Target o{};
    o.p = nv12_dev; o.frame_stride = desc->frame_stride; o.uv_offset = desc->uv_offset; o.pitch = desc->pitch;
    o.y_dwords = (uintptr_t)nv12_dev % 4 == 0 && desc->pitch % 4 == 0 && desc->frame_stride % 4 == 0;
    o.uv_dwords = o.y_dwords && desc->uv_offset % 4 == 0;
    fid_yuv_fwd_for(desc->standard, &o.k);
    hipLaunchKernelGGL(draw_paint_nv12, dim3(grid), dim3(256), 0, ctx->stream, o, (const int32_t *)a.nb, (const int4 *)a.ext,
                       (const uint32_t *)a.rec, H, W, cap, ntx, (int)tiles_per_frame, total, (style->thickness - 1) / 2, style->text_scale);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_draw_faces_nv12_host(uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, const float *det, const int32_t *counts, int cap,
                             const int32_t *idx, const float *score, int id_stride, const int32_t *offsets, int n_rows, const int32_t *track,
                             const char *names, const int32_t *name_offsets, const uint8_t *bgr, int G, const fid_draw_style *style) {
    FID_TRY(check_draw(nv12, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, style));
    FID_TRY(check_nv12(desc, B, H, W));
    std::vector<fid_draw_label> tab;
    if (name_offsets) FID_TRY(make_labels(names, name_offsets, bgr, G, tab));
    const int nG = (int)tab.size(), r = (style->thickness - 1) / 2, t = style->text_scale;
    fid_yuv_fwd k;
    fid_yuv_fwd_for(desc->standard, &k);
    if (!idx) offsets = nullptr;
    for (int b = 0; b < B; b++) {
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, idx != nullptr, id_stride, offsets, n_rows, &row0);
        uint8_t *yp = nv12 + (size_t)b * (size_t)desc->frame_stride;
        for (int f = 0; f < n; f++) {          // ascending: a later face overwrites an earlier one, pixel by pixel and pair by pair
            const size_t slot = (size_t)b * cap + f;
            int ii = -1;
            float sc = 0.f;
            if (idx) {
                const size_t i = offsets ? (size_t)row0 + f : (size_t)b * id_stride + f;
                ii = idx[i]; sc = score[i];
            }
            const bool known = ii >= 0 && ii < nG;
            fid_draw_face fc;
            fid_draw_make_face(&fc, det + slot * 5, known ? &tab[ii] : nullptr, sc, track ? track[slot * 2] : -1, style, H, W);
            fid_draw_face_nv12_host(&fc, k, yp, yp + desc->uv_offset, desc->pitch, r, t, h_font);
        }
    }
    return FID_OK;
}

int fid_draw_glyphs(uint8_t *out) {
    FID_REQUIRE(out, "draw glyphs: NULL output");
    memcpy(out, h_font, sizeof(h_font));
    return FID_OK;
}

}  // extern "C"
