// Redacting faces on the frames, on the device: a mosaic or a solid fill over every selected face, enqueued behind the match with nothing
// read back first (include/faceid.h, fid_redact_faces).  The arithmetic -- face record, cell rectangle, mean, FILL values, the per-face cell
// bound -- is redact_core.h's, shared with the host twins below.
//
// The same shape of problem as draw.hip: where two regions overlap the LATER face shows, so the write is a gather per tile, not one
// workgroup per face.  And every mean is taken from the frame as it was before the call, so the means are a launch of their own that the
// stream orders in front of the writes.  Three kernels per call (FILL: the first and the last):
//
//   redact_prepare  one thread per (frame, face slot): the face record into a [B, cap] table in the context's scratch, its clipped region
//                   into a table of its own (16 bytes per face: what the cull reads; an unselected or invalid face gets the empty extent),
//                   and the frame's face count.
//   redact_means    one workgroup per face slot; an empty slot returns at once.  The four waves take the cells that meet the clipped region;
//                   the lanes stride along the rows of the cell (a cell narrower than a wave is walked as one run of pixels instead), so
//                   loads run along x.  Per-lane uint32 partial sums: a lane's share is at most H * W / 64 < 2^31 / 3 / 64 < 2^24 pixels of
//                   at most 255, below 2^32.  The wave reduction and the division are 64-bit.  Lane 0 stores the packed value (B, G, R or
//                   Y, U, V) into the face's row of the cell table: plain vector stores, no atomics.
//   redact_paint    draw_paint's 64 x 16 tiles, cull by ballot + popcount, ascending list.  Each thread owns four adjacent pixels of one
//                   row and keeps, per pixel, the last listed face whose clipped region contains it and that face's cell; one table read
//                   per covered pixel.  Covered pixels only are stored; four covered pixels in dword-aligned rows are dword stores.  NV12:
//                   Y per pixel, one pair per group from the group's own first pixel -- regions and cells are 2 x 2 aligned, so a group
//                   never straddles two of them and no lane exchange is needed.
//
// This file must never get a fast-math flag: the margin is one double multiply truncated to int, compared bit for bit with the host's.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "redact_core.h"

namespace {

using fid::cdiv;

constexpr int TILE_W = 64, TILE_H = 16;
constexpr int MAX_GRID = 1 << 18;
constexpr int REC_CHUNK = 64;               // records in LDS at a time: 3 KB

struct PrepArgs {
    const float *det;
    const int32_t *counts, *idx, *offsets;
    int B, cap, id_stride, n_rows, H, W;
    fid_redact_style st;
    int32_t *nb;                             // [B] faces of frame b
    int4 *ext;                               // [B, cap] clipped regions (x0, y0, x1, y1), x0 > x1: nothing
    fid_redact_face *rec;                    // [B, cap]
    uint32_t *tab;                           // [B, cap, bound] cell values (MOSAIC)
    int bound;
};

__global__ void __launch_bounds__(256) redact_prepare(const PrepArgs a) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)a.B * a.cap) return;
    const int b = (int)(gid / a.cap), f = (int)(gid % a.cap);
    int row0;
    const int n = fid_draw_face_count(b, a.counts, a.cap, a.idx != nullptr, a.id_stride, a.offsets, a.n_rows, &row0);
    if (f == 0) a.nb[b] = n;
    bool selected = false;
    if (f < n) {
        int ii = -1;
        if (a.idx) ii = a.idx[a.offsets ? (long long)row0 + f : (long long)b * a.id_stride + f];
        selected = fid_redact_selected(a.st.who, a.idx != nullptr, ii);
    }
    fid_redact_face fc;
    fid_redact_make_face(&fc, a.det + gid * 5, selected, &a.st, a.H, a.W);
    a.rec[gid] = fc;
    a.ext[gid] = make_int4(fc.x0, fc.y0, fc.x1, fc.y1);
}

// the frames a kernel reads or writes: dense BGR (p, dwords) or NV12 in a layout
struct Target {
    uint8_t *p;
    long long frame_stride, uv_offset;
    int pitch, y_dwords, uv_dwords;          // BGR: y_dwords = rows are dword-aligned
};

__device__ __forceinline__ uint64_t wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// sums of the bytes at base + (y * row_stride + x * step + k), k < NCH, over x < cw, y < ch, per lane
template <int NCH>
__device__ __forceinline__ void cell_sums(const uint8_t *base, size_t row_stride, int step, int cw, int ch, int lane, uint32_t *s) {
    if (cw >= 64) {
        for (int y = 0; y < ch; y++) {
            const uint8_t *row = base + (size_t)y * row_stride;
            for (int x = lane; x < cw; x += 64) {
#pragma unroll
                for (int k = 0; k < NCH; k++) s[k] += row[(size_t)x * step + k];
            }
        }
    } else {
        const int n = cw * ch;                                  // (below H * W)
        for (int i = lane; i < n; i += 64) {
            const int y = (int)((unsigned)i / (unsigned)cw), x = i - y * cw;
            const uint8_t *p = base + (size_t)y * row_stride + (size_t)x * step;
#pragma unroll
            for (int k = 0; k < NCH; k++) s[k] += p[k];
        }
    }
}

template <bool NV12>
__global__ void __launch_bounds__(256) redact_means(const Target o, const fid_redact_face *__restrict__ rec, uint32_t *__restrict__ tab, int bound,
                                                    int cap, int H, int W) {
    const size_t slot = blockIdx.x;
    const fid_redact_face fc = rec[slot];
    if (!fc.sel) return;                     // (block-uniform)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = (int)(slot / (size_t)cap);
    const int i0 = (fc.x0 - fc.ax) / fc.c, i1 = (fc.x1 - fc.ax) / fc.c, j0 = (fc.y0 - fc.ay) / fc.c, j1 = (fc.y1 - fc.ay) / fc.c;
    const int nx = i1 - i0 + 1, nvis = nx * (j1 - j0 + 1);      // the cells that meet the clipped region: at most ncx * ncy <= bound
    const uint8_t *frame = o.p + (size_t)b * (size_t)o.frame_stride;
    for (int k = wave; k < nvis; k += 4) {   // (wave-uniform)
        const int j = j0 + k / nx, i = i0 + k % nx;
        int r[4];
        if (!fid_redact_cell_rect(&fc, i, j, r)) continue;
        const int cw = r[2] - r[0] + 1, ch = r[3] - r[1] + 1;
        const uint64_t cnt = (uint64_t)cw * (uint64_t)ch;
        uint32_t s[3] = {0u, 0u, 0u};
        uint64_t t0, t1, t2, cn = cnt;
        if (NV12) {
            cell_sums<1>(frame + (size_t)r[1] * o.pitch + r[0], (size_t)o.pitch, 1, cw, ch, lane, s);
            cell_sums<2>(frame + (size_t)o.uv_offset + (size_t)(r[1] >> 1) * o.pitch + r[0], (size_t)o.pitch, 2, cw >> 1, ch >> 1, lane, s + 1);
            cn = cnt >> 2;                   // (cw and ch are even: whole groups)
        } else {
            cell_sums<3>(frame + ((size_t)r[1] * W + r[0]) * 3, (size_t)W * 3, 3, cw, ch, lane, s);
        }
        t0 = wave_sum(s[0]); t1 = wave_sum(s[1]); t2 = wave_sum(s[2]);
        if (lane == 0)
            tab[slot * (size_t)bound + (size_t)(j * fc.ncx + i)] =
                fid_redact_pack(fid_redact_mean(t0, cnt), fid_redact_mean(t1, cn), fid_redact_mean(t2, cn));
    }
}

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

template <bool NV12>
__global__ void __launch_bounds__(256) redact_paint(const Target o, const int32_t *__restrict__ nb, const int4 *__restrict__ ext,
                                                    const uint32_t *__restrict__ rec, const uint32_t *__restrict__ tab, int bound, uint32_t fill,
                                                    int mosaic, int H, int W, int cap, int ntx, int tiles_per_frame, long long total_tiles) {
    __shared__ uint32_t s_rec[REC_CHUNK * FID_REDACT_FACE_WORDS];
    __shared__ int s_list[256];
    __shared__ int s_wcount[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_frame), rem = (int)(tile % tiles_per_frame);
        const int X0 = (rem % ntx) * TILE_W, Y0 = (rem / ntx) * TILE_H;
        const int X1 = min(X0 + TILE_W - 1, W - 1), Y1 = min(Y0 + TILE_H - 1, H - 1);
        const int px = X0 + (tid & 15) * 4, py = Y0 + (tid >> 4);
        const int n = nb[b];
        int win[4] = {-1, -1, -1, -1};       // the last listed face whose clipped region holds pixel p; -1: not covered
        int cell[4] = {0, 0, 0, 0};          // ... and the pixel's cell in that face's row of the table
        for (int f0 = 0; f0 < n; f0 += 256) {
            const int f = f0 + tid;
            bool hit = false;
            if (f < n) {
                const int4 e = ext[(size_t)b * cap + f];
                hit = e.x <= e.z && e.x <= X1 && e.z >= X0 && e.y <= Y1 && e.w >= Y0;
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
                for (int i = tid; i < nrec * FID_REDACT_FACE_WORDS; i += 256) {
                    const int j = i / FID_REDACT_FACE_WORDS, k = i - j * FID_REDACT_FACE_WORDS;
                    s_rec[i] = rec[((size_t)b * cap + s_list[j0 + j]) * FID_REDACT_FACE_WORDS + k];
                }
                __syncthreads();
                if (py <= Y1) {
                    for (int j = 0; j < nrec; j++) {
                        const fid_redact_face *fc = (const fid_redact_face *)(s_rec + j * FID_REDACT_FACE_WORDS);
                        if (py < fc->y0 || py > fc->y1 || px + 3 < fc->x0 || px > fc->x1) continue;
                        const int fi = s_list[j0 + j];
                        // px and the anchor are even and c is even: pixels 0, 1 share a cell, and so do pixels 2, 3
                        const unsigned c = (unsigned)fc->c;
                        const int row = (int)((unsigned)(py - fc->ay) / c) * fc->ncx;
                        const int ca = row + (int)((unsigned)(px - fc->ax) / c), cb = row + (int)((unsigned)(px + 2 - fc->ax) / c);
#pragma unroll
                        for (int p = 0; p < 4; p++)
                            if (px + p >= fc->x0 && px + p <= fc->x1) { win[p] = fi; cell[p] = p < 2 ? ca : cb; }
                    }
                }
                __syncthreads();             // the next chunk, pass or tile rewrites s_rec / s_list
            }
        }
        unsigned cov = 0u;
        uint32_t v[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            v[p] = fill;
            if (win[p] >= 0) {
                cov |= 1u << p;
                if (mosaic) v[p] = tab[((size_t)b * cap + win[p]) * (size_t)bound + cell[p]];
            }
        }
        if (cov == 0u) continue;             // (a covered pixel lies inside the frame: regions are clipped to it)
        if (!NV12) {
            uint8_t *dst = o.p + (((size_t)b * H + py) * W + px) * 3;
            if (cov == 15u && o.y_dwords) {
                uint32_t *d = (uint32_t *)dst;
                d[0] = v[0] | (v[1] << 24);
                d[1] = (v[1] >> 8) | (v[2] << 16);
                d[2] = (v[2] >> 16) | (v[3] << 8);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (cov & (1u << p)) { dst[p * 3] = (uint8_t)v[p]; dst[p * 3 + 1] = (uint8_t)(v[p] >> 8); dst[p * 3 + 2] = (uint8_t)(v[p] >> 16); }
            }
        } else {
            uint8_t *frame = o.p + (size_t)b * (size_t)o.frame_stride;
            uint8_t *dst = frame + (size_t)py * o.pitch + px;
            if (cov == 15u && o.y_dwords) {
                *(uint32_t *)dst = (v[0] & 255u) | ((v[1] & 255u) << 8) | ((v[2] & 255u) << 16) | ((v[3] & 255u) << 24);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (cov & (1u << p)) dst[p] = (uint8_t)v[p];
            }
            if ((py & 1) == 0) {             // the even row of a group stores its pair: W is even, a covered pixel 0 (2) has its whole group covered
                uint8_t *uv = frame + (size_t)o.uv_offset + (size_t)(py >> 1) * o.pitch + px;
                if ((cov & 5u) == 5u && o.uv_dwords) {
                    *(uint32_t *)uv = ((v[0] >> 8) & 0xFFFFu) | (((v[2] >> 8) & 0xFFFFu) << 16);
                } else {
                    if (cov & 1u) { uv[0] = (uint8_t)(v[0] >> 8); uv[1] = (uint8_t)(v[0] >> 16); }
                    if (cov & 4u) { uv[2] = (uint8_t)(v[2] >> 8); uv[3] = (uint8_t)(v[2] >> 16); }
                }
            }
        }
    }
}

int check_redact(const void *frames, int B, int H, int W, const void *det, const void *counts, int cap, const void *idx, const void *score,
                 int id_stride, const void *offsets, int n_rows, const fid_redact_style *st) {
    const char *why = fid_redact_check(frames, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, st);
    FID_REQUIRE(why == nullptr, "redact: %s", why ? why : "");
    return FID_OK;
}

int check_nv12(const fid_nv12_desc *desc, int B, int H, int W) {
    const char *why = fid_nv12_check(desc, B, H, W);
    FID_REQUIRE(why == nullptr, "redact: nv12: %s", why ? why : "");
    return FID_OK;
}

// the three launches of a call, BGR or NV12 (the context's lock is held, its device is set)
template <bool NV12>
int redact_launch(fid_ctx *ctx, const Target &o, uint32_t fill, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap,
                  const int32_t *idx_dev, int id_stride, const int32_t *offsets_dev, int n_rows, const fid_redact_style *style) {
    const size_t faces = (size_t)B * cap;
    const bool mosaic = style->mode == FID_REDACT_MOSAIC;
    const int bound = fid_redact_cell_bound(style->cells, style->expand);
    const size_t off_ext = ((size_t)B * 4 + 15) & ~(size_t)15, off_rec = off_ext + faces * sizeof(int4);
    const size_t off_tab = off_rec + faces * sizeof(fid_redact_face);
    void *ws;
    FID_TRY(fid::get_scratch(ctx, 2, off_tab + (mosaic ? faces * (size_t)bound * sizeof(uint32_t) : 0), &ws));
    PrepArgs a{};
    a.det = det_dev; a.counts = counts_dev; a.idx = idx_dev; a.offsets = idx_dev ? offsets_dev : nullptr;
    a.B = B; a.cap = cap; a.id_stride = id_stride; a.n_rows = n_rows; a.H = H; a.W = W;
    a.st = *style;
    a.nb = (int32_t *)ws; a.ext = (int4 *)((char *)ws + off_ext); a.rec = (fid_redact_face *)((char *)ws + off_rec);
    a.tab = (uint32_t *)((char *)ws + off_tab); a.bound = bound;
    hipLaunchKernelGGL(redact_prepare, dim3((unsigned)fid::cdiv64((int64_t)faces, 256)), dim3(256), 0, ctx->stream, a);
    if (mosaic)
        hipLaunchKernelGGL(redact_means<NV12>, dim3((unsigned)faces), dim3(256), 0, ctx->stream, o, (const fid_redact_face *)a.rec, a.tab, bound, cap,
                           H, W);
    const int ntx = cdiv(W, TILE_W), nty = cdiv(H, TILE_H);
    const long long tiles_per_frame = (long long)ntx * nty, total = tiles_per_frame * B;      // (H * W * 3 fits int32: so does ntx * nty)
    const int grid = (int)std::min<long long>(total, MAX_GRID);
    hipLaunchKernelGGL(redact_paint<NV12>, dim3(grid), dim3(256), 0, ctx->stream, o, (const int32_t *)a.nb, (const int4 *)a.ext,
                       (const uint32_t *)a.rec, (const uint32_t *)a.tab, bound, fill, mosaic ? 1 : 0, H, W, cap, ntx, (int)tiles_per_frame, total);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // namespace

extern "C" {

int fid_redact_faces(fid_ctx *ctx, uint8_t *frames_dev, int B, int H, int W, const float *det_dev, const int32_t *counts_dev, int cap,
                     const int32_t *idx_dev, const float *score_dev, int id_stride, const int32_t *offsets_dev, int n_rows,
                     const fid_redact_style *style) {
    FID_REQUIRE(ctx, "redact: NULL context");
    FID_TRY(check_redact(frames_dev, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, style));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    Target o{};
    o.p = frames_dev; o.frame_stride = (long long)H * W * 3;
    o.y_dwords = (W % 4 == 0) && ((uintptr_t)frames_dev % 4 == 0);
    return redact_launch<false>(ctx, o, fid_redact_fill_bgr(style), B, H, W, det_dev, counts_dev, cap, idx_dev, id_stride, offsets_dev, n_rows, style);
}

int fid_redact_faces_host(uint8_t *frames, int B, int H, int W, const float *det, const int32_t *counts, int cap, const int32_t *idx,
                          const float *score, int id_stride, const int32_t *offsets, int n_rows, const fid_redact_style *style) {
    FID_TRY(check_redact(frames, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, style));
    if (!fid_redact_frames_host(frames, B, H, W, det, counts, cap, idx, id_stride, offsets, n_rows, style)) {
        fid::set_error("redact: out of host memory for the cell table of %d face slots", cap);
        return FID_E_NOMEM;
    }
    return FID_OK;
}

int fid_redact_faces_nv12(fid_ctx *ctx, uint8_t *nv12_dev, const fid_nv12_desc *desc, int B, int H, int W, const float *det_dev,
                          const int32_t *counts_dev, int cap, const int32_t *idx_dev, const float *score_dev, int id_stride,
                          const int32_t *offsets_dev, int n_rows, const fid_redact_style *style) {
    FID_REQUIRE(ctx, "redact: NULL context");
    FID_TRY(check_redact(nv12_dev, B, H, W, det_dev, counts_dev, cap, idx_dev, score_dev, id_stride, offsets_dev, n_rows, style));
    FID_TRY(check_nv12(desc, B, H, W));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));
    Target o{};
    o.p = nv12_dev; o.frame_stride = desc->frame_stride; o.uv_offset = desc->uv_offset; o.pitch = desc->pitch;
    o.y_dwords = (uintptr_t)nv12_dev % 4 == 0 && desc->pitch % 4 == 0 && desc->frame_stride % 4 == 0;
    o.uv_dwords = o.y_dwords && desc->uv_offset % 4 == 0;
    fid_yuv_fwd k;
    fid_yuv_fwd_for(desc->standard, &k);
    return redact_launch<true>(ctx, o, fid_redact_fill_yuv(style, k), B, H, W, det_dev, counts_dev, cap, idx_dev, id_stride, offsets_dev, n_rows, style);
}

int fid_redact_faces_nv12_host(uint8_t *nv12, const fid_nv12_desc *desc, int B, int H, int W, const float *det, const int32_t *counts, int cap,
                               const int32_t *idx, const float *score, int id_stride, const int32_t *offsets, int n_rows,
                               const fid_redact_style *style) {
    FID_TRY(check_redact(nv12, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, style));
    FID_TRY(check_nv12(desc, B, H, W));
    if (!fid_redact_frames_nv12_host(nv12, desc, B, H, W, det, counts, cap, idx, id_stride, offsets, n_rows, style)) {
        fid::set_error("redact: out of host memory for the cell table of %d face slots", cap);
        return FID_E_NOMEM;
    }
    return FID_OK;
}

}  // extern "C"
