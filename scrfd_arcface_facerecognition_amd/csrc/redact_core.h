// The redaction's arithmetic, once, for the device kernels (redact.hip), the host twins (fid_redact_faces_host, fid_redact_faces_nv12_host)
// and the stand-alone sanitizer driver (tests/redact_host_driver.cpp): the face record (selected, anchor, cell size, cell counts, clipped
// region), the rectangle and the mean of a cell, the FILL values, the per-face cell bound, the argument checks, and the two host loops.
// Integer arithmetic only (the margin is one double multiply, truncated), so device, host and a numpy restatement agree to the byte.  Plain
// inline functions, no HIP runtime call; compiles with a host-only compiler.  The definition is include/faceid.h's (fid_redact_faces); nothing
// here is the reference's, which shows every face in the clear.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "draw_core.h"
#include "yuv_core.h"

// one face of one frame, ready for the means and the paint
struct fid_redact_face {
    int32_t sel;                   // 1: selected, valid, and its clipped region is not empty; 0: the face redacts nothing
    int32_t ax, ay;                // anchor of the cell grid: the UNCLIPPED rx0, ry0 (even)
    int32_t c;                     // cell edge (even, >= 2)
    int32_t ncx, ncy;              // cells of the unclipped region along x and y; ncx * ncy <= fid_redact_cell_bound(cells, expand)
    int32_t x0, y0, x1, y1;        // the region clipped to the frame, inclusive
    int32_t pad_[2];
};
#define FID_REDACT_FACE_WORDS 12
static_assert(sizeof(fid_redact_face) == 4 * FID_REDACT_FACE_WORDS, "fid_redact_face is copied as 12 dwords");

// Cells one face can have, from (cells, expand) alone: what the cell table holds per face slot.
// Along x the unclipped region is R = rx1 - rx0 + 1 <= w + 2 * mx + 3 wide (rx0 >= x1 - mx - 1, rx1 <= x2 + mx + 1), with mx <= expand * w and
// w <= s = max(w, h); likewise along y.  q = s / cells (integer), so s <= cells * (q + 1) - 1, and c = max(2, q rounded up to even) has
// (q + 1) / c <= 3 / 2 (reached at q = 2, c = 2) and 3 / c <= 1.5.  Hence
//   R / c <= (1 + 2 * expand) * (cells * (q + 1) - 1) / c + 3 / c  <  1.5 * (1 + 2 * expand) * cells + 1.5,
// and ceil(R / c) <= floor(1.5 * (1 + 2 * expand) * cells) + 2.  One more cell absorbs the rounding of the double product.  At the defaults
// (8, 0.1) that is 17 per axis, 289 per face; at (16, 0.5) 51 per axis, 2601 per face.  tests/test_redact_cpu.py enumerates w, h in 1 .. 200.
FID_HD int fid_redact_cells_per_axis(int cells, double expand) { return (int)(1.5 * (1.0 + 2.0 * expand) * (double)cells) + 3; }
FID_HD int fid_redact_cell_bound(int cells, double expand) {
    const int n = fid_redact_cells_per_axis(cells, expand);
    return n * n;
}

// The record of one face.  d: its det row (x1, y1, x2, y2, conf); selected: `who` has the bit of the face's class.
FID_HD void fid_redact_make_face(fid_redact_face *o, const float *d, bool selected, const fid_redact_style *st, int H, int W) {
    o->sel = 0; o->ax = o->ay = 0; o->c = 2; o->ncx = o->ncy = 0;
    o->x0 = 1; o->y0 = 1; o->x1 = 0; o->y1 = 0; o->pad_[0] = o->pad_[1] = 0;
    if (!selected) return;
    for (int i = 0; i < 4; i++)
        if (!(fabsf(d[i]) < 8388608.f)) return;                 // NaN, infinity, |v| >= 2^23
    const int x1 = (int)d[0], y1 = (int)d[1], x2 = (int)d[2], y2 = (int)d[3];
    const int w = x2 - x1, h = y2 - y1;                         // (below 2^24)
    if (!(w > 0 && h > 0)) return;
    const int mx = (int)(st->expand * (double)w), my = (int)(st->expand * (double)h);
    const int rx0 = (x1 - mx) & ~1, rx1 = (x2 + mx) | 1;        // (& ~1 on a two's complement negative is the floor to even)
    const int ry0 = (y1 - my) & ~1, ry1 = (y2 + my) | 1;        // (every term stays below 2^25)
    const int s = fid_draw_imax(w, h);
    const int c = fid_draw_imax(2, (s / st->cells + 1) & ~1);
    o->ax = rx0; o->ay = ry0; o->c = c;
    o->ncx = (rx1 - rx0 + c) / c; o->ncy = (ry1 - ry0 + c) / c;
    const int cx0 = fid_draw_imax(rx0, 0), cy0 = fid_draw_imax(ry0, 0), cx1 = fid_draw_imin(rx1, W - 1), cy1 = fid_draw_imin(ry1, H - 1);
    if (cx0 > cx1 || cy0 > cy1) return;                         // wholly outside the frame
    o->x0 = cx0; o->y0 = cy0; o->x1 = cx1; o->y1 = cy1;
    o->sel = 1;
}

// cell (i, j) of a selected face, intersected with its clipped region: r = (xa, ya, xb, yb) inclusive; false: empty
FID_HD bool fid_redact_cell_rect(const fid_redact_face *fc, int i, int j, int *r) {
    r[0] = fid_draw_imax(fc->ax + i * fc->c, fc->x0); r[2] = fid_draw_imin(fc->ax + (i + 1) * fc->c - 1, fc->x1);
    r[1] = fid_draw_imax(fc->ay + j * fc->c, fc->y0); r[3] = fid_draw_imin(fc->ay + (j + 1) * fc->c - 1, fc->y1);
    return r[0] <= r[2] && r[1] <= r[3];
}

// the cell of pixel (x, y) of the clipped region, as an index into the face's ncx * ncy table entries
FID_HD int fid_redact_cell_of(const fid_redact_face *fc, int x, int y) {
    return (int)((unsigned)(y - fc->ay) / (unsigned)fc->c) * fc->ncx + (int)((unsigned)(x - fc->ax) / (unsigned)fc->c);
}

// the mean of n > 0 bytes that sum to `sum`: integer division, half rounds up
FID_HD uint32_t fid_redact_mean(uint64_t sum, uint64_t n) { return (uint32_t)((sum + n / 2) / n); }

FID_HD uint32_t fid_redact_pack(uint32_t a, uint32_t b, uint32_t c) { return a | (b << 8) | (c << 16); }

// is the face of identity entry ii (any value without an idx array) selected?
FID_HD bool fid_redact_selected(int who, bool has_idx, int ii) {
    return (who & ((has_idx && ii >= 0) ? FID_REDACT_KNOWN : FID_REDACT_UNKNOWN)) != 0;
}

// the FILL colour as a table entry: (B, G, R), or for NV12 (Y, U, V) as fid_draw_faces_nv12 colours a pixel
FID_HD uint32_t fid_redact_fill_bgr(const fid_redact_style *st) { return fid_redact_pack(st->fill_bgr[0], st->fill_bgr[1], st->fill_bgr[2]); }
FID_HD uint32_t fid_redact_fill_yuv(const fid_redact_style *st, const fid_yuv_fwd &k) {
    int yuv[3];
    fid_yuv_of_colour(k, st->fill_bgr[0], st->fill_bgr[1], st->fill_bgr[2], yuv);
    return fid_redact_pack((uint32_t)yuv[0], (uint32_t)yuv[1], (uint32_t)yuv[2]);
}

// argument checks shared by the device and the host entry points; NULL = fine, else what is wrong.  The shared arguments are checked by
// fid_draw_check itself (with a style it accepts), so that the two calls refuse the same things.
inline const char *fid_redact_check(const void *frames, long long B, long long H, long long W, const void *det, const void *counts, long long cap,
                                    const void *idx, const void *score, int id_stride, const void *offsets, int n_rows, const fid_redact_style *st) {
    fid_draw_style ok;
    ok.proportion = 0.2; ok.thickness = 3; ok.text_scale = 0; ok.bar = 0; ok.flags = 0;
    ok.unknown_bgr[0] = ok.unknown_bgr[1] = ok.unknown_bgr[2] = ok.unknown_bgr[3] = 0;
    if (!st) return "a NULL style";
    const char *why = fid_draw_check(frames, B, H, W, det, counts, cap, idx, score, id_stride, offsets, n_rows, &ok);
    if (why) return why;
    if (st->mode != FID_REDACT_MOSAIC && st->mode != FID_REDACT_FILL) return "an unknown mode";
    if (st->who < 1 || st->who > 3) return "who outside 1 .. 3";
    if (st->cells < 1 || st->cells > 16) return "cells outside 1 .. 16";
    if (!(st->expand >= 0.0 && st->expand <= 0.5)) return "expand NaN or outside [0, 0.5]";
    if (st->reserved != 0) return "reserved must be 0";
    return nullptr;
}

// ---- the host twins' loops: the table of cell values first, the writes second ----

// the records of frame b's n faces into rec [n] and the first table entry of each into first [n + 1]
inline void fid_redact_frame_faces(fid_redact_face *rec, uint32_t *first, int b, int n, int row0, const float *det, int cap, const int32_t *idx,
                                   int id_stride, const int32_t *offsets, const fid_redact_style *st, int H, int W) {
    first[0] = 0;
    for (int f = 0; f < n; f++) {
        const size_t slot = (size_t)b * cap + f;
        int ii = -1;
        if (idx) ii = idx[offsets ? (size_t)row0 + f : (size_t)b * id_stride + f];
        fid_redact_make_face(&rec[f], det + slot * 5, fid_redact_selected(st->who, idx != nullptr, ii), st, H, W);
        first[f + 1] = first[f] + (rec[f].sel ? (uint32_t)(rec[f].ncx * rec[f].ncy) : 0u);
    }
}

// B dense BGR frames [B,H,W,3] in place (the arguments have passed fid_redact_check); false: out of host memory, nothing written
inline bool fid_redact_frames_host(uint8_t *frames, int B, int H, int W, const float *det, const int32_t *counts, int cap, const int32_t *idx,
                                   int id_stride, const int32_t *offsets, int n_rows, const fid_redact_style *st) {
    if (!idx) offsets = nullptr;
    fid_redact_face *rec = (fid_redact_face *)malloc((size_t)cap * sizeof(fid_redact_face));
    uint32_t *first = (uint32_t *)malloc(((size_t)cap + 1) * sizeof(uint32_t));
    uint32_t *tab = (uint32_t *)malloc((size_t)cap * (size_t)fid_redact_cell_bound(st->cells, st->expand) * sizeof(uint32_t));
    if (!rec || !first || !tab) { free(rec); free(first); free(tab); return false; }
    const uint32_t fill = fid_redact_fill_bgr(st);
    for (int b = 0; b < B; b++) {
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, idx != nullptr, id_stride, offsets, n_rows, &row0);
        uint8_t *img = frames + (size_t)b * H * W * 3;
        fid_redact_frame_faces(rec, first, b, n, row0, det, cap, idx, id_stride, offsets, st, H, W);
        if (st->mode == FID_REDACT_MOSAIC)
            for (int f = 0; f < n; f++) {      // every mean from the frame as it was before the call
                if (!rec[f].sel) continue;
                for (int j = 0; j < rec[f].ncy; j++)
                    for (int i = 0; i < rec[f].ncx; i++) {
                        int r[4];
                        if (!fid_redact_cell_rect(&rec[f], i, j, r)) continue;
                        uint64_t s[3] = {0, 0, 0};
                        for (int y = r[1]; y <= r[3]; y++)
                            for (int x = r[0]; x <= r[2]; x++) {
                                const uint8_t *p = img + ((size_t)y * W + x) * 3;
                                s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
                            }
                        const uint64_t cnt = (uint64_t)(r[2] - r[0] + 1) * (uint64_t)(r[3] - r[1] + 1);
                        tab[first[f] + (uint32_t)(j * rec[f].ncx + i)] =
                            fid_redact_pack(fid_redact_mean(s[0], cnt), fid_redact_mean(s[1], cnt), fid_redact_mean(s[2], cnt));
                    }
            }
        for (int f = 0; f < n; f++) {          // ascending: the highest face index shows
            if (!rec[f].sel) continue;
            for (int y = rec[f].y0; y <= rec[f].y1; y++)
                for (int x = rec[f].x0; x <= rec[f].x1; x++) {
                    const uint32_t v = st->mode == FID_REDACT_MOSAIC ? tab[first[f] + (uint32_t)fid_redact_cell_of(&rec[f], x, y)] : fill;
                    uint8_t *p = img + ((size_t)y * W + x) * 3;
                    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
                }
        }
    }
    free(tab); free(first); free(rec);
    return true;
}

// B NV12 frames in the layout d in place (the arguments have passed fid_redact_check and fid_nv12_check).  H and W are even, the region and
// the cells are even-aligned with an even size: a clipped cell holds whole 2 x 2 groups only.
inline bool fid_redact_frames_nv12_host(uint8_t *nv12, const fid_nv12_desc *d, int B, int H, int W, const float *det, const int32_t *counts,
                                        int cap, const int32_t *idx, int id_stride, const int32_t *offsets, int n_rows,
                                        const fid_redact_style *st) {
    fid_yuv_fwd k;
    if (!fid_yuv_fwd_for(d->standard, &k)) return false;
    if (!idx) offsets = nullptr;
    fid_redact_face *rec = (fid_redact_face *)malloc((size_t)cap * sizeof(fid_redact_face));
    uint32_t *first = (uint32_t *)malloc(((size_t)cap + 1) * sizeof(uint32_t));
    uint32_t *tab = (uint32_t *)malloc((size_t)cap * (size_t)fid_redact_cell_bound(st->cells, st->expand) * sizeof(uint32_t));
    if (!rec || !first || !tab) { free(rec); free(first); free(tab); return false; }
    const uint32_t fill = fid_redact_fill_yuv(st, k);
    const size_t pitch = (size_t)d->pitch;
    for (int b = 0; b < B; b++) {
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, idx != nullptr, id_stride, offsets, n_rows, &row0);
        uint8_t *yp = nv12 + (size_t)b * (size_t)d->frame_stride, *uvp = yp + d->uv_offset;
        fid_redact_frame_faces(rec, first, b, n, row0, det, cap, idx, id_stride, offsets, st, H, W);
        if (st->mode == FID_REDACT_MOSAIC)
            for (int f = 0; f < n; f++) {
                if (!rec[f].sel) continue;
                for (int j = 0; j < rec[f].ncy; j++)
                    for (int i = 0; i < rec[f].ncx; i++) {
                        int r[4];
                        if (!fid_redact_cell_rect(&rec[f], i, j, r)) continue;
                        uint64_t s[3] = {0, 0, 0};
                        for (int y = r[1]; y <= r[3]; y++)
                            for (int x = r[0]; x <= r[2]; x++) s[0] += yp[(size_t)y * pitch + (size_t)x];
                        for (int y = r[1]; y <= r[3]; y += 2)
                            for (int x = r[0]; x <= r[2]; x += 2) {
                                const uint8_t *c = uvp + (size_t)(y >> 1) * pitch + (size_t)x;
                                s[1] += c[0]; s[2] += c[1];
                            }
                        const uint64_t cnt = (uint64_t)(r[2] - r[0] + 1) * (uint64_t)(r[3] - r[1] + 1);
                        tab[first[f] + (uint32_t)(j * rec[f].ncx + i)] =
                            fid_redact_pack(fid_redact_mean(s[0], cnt), fid_redact_mean(s[1], cnt / 4), fid_redact_mean(s[2], cnt / 4));
                    }
            }
        for (int f = 0; f < n; f++) {
            if (!rec[f].sel) continue;
            for (int y = rec[f].y0; y <= rec[f].y1; y++)
                for (int x = rec[f].x0; x <= rec[f].x1; x++) {
                    const uint32_t v = st->mode == FID_REDACT_MOSAIC ? tab[first[f] + (uint32_t)fid_redact_cell_of(&rec[f], x, y)] : fill;
                    yp[(size_t)y * pitch + (size_t)x] = (uint8_t)v;
                    if (!(y & 1) && !(x & 1)) {
                        uint8_t *c = uvp + (size_t)(y >> 1) * pitch + (size_t)x;
                        c[0] = (uint8_t)(v >> 8); c[1] = (uint8_t)(v >> 16);
                    }
                }
        }
    }
    free(tab); free(first); free(rec);
    return true;
}
