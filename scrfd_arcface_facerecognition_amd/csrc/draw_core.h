// The overlay's arithmetic, once, for the device kernels (draw.hip), the host rasteriser (fid_draw_faces_host) and the stand-alone
// sanitizer driver (tests/draw_host_driver.cpp): the face record, its label text, the per-pixel coverage test, the three identity
// forms.  Plain inline functions, no HIP runtime call; compiles with a host-only compiler.
//
// What is the reference's (utils/helpers.py:126-179, main.py:130-148): integer truncation of the box, the corner length, the bar
// rectangle, the text anchor, the label string and its two decimals, the unknown colour, the draw order.  What is this project's own:
// the raster of a thick segment (every point stamps a thickness x thickness square) and the 5 x 7 font below.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/faceid.h"

#if defined(__HIPCC__)
#define FID_HD __host__ __device__ inline
#else
#define FID_HD inline
#endif

// 95 glyphs, ASCII 0x20 .. 0x7E, 7 rows each, top row first; bit 4 = leftmost column, bit 0 = rightmost
#define FID_DRAW_GLYPHS 95
#define FID_DRAW_FONT_INIT                                                                                                   \
    {                                                                                                                        \
        0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, /*   */ 0x04, 0x04, 0x04, 0x04, 0x04, 0x00, 0x04, /* ! */                  \
        0x0A, 0x0A, 0x0A, 0x00, 0x00, 0x00, 0x00, /* " */ 0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A, /* # */                  \
        0x04, 0x0F, 0x14, 0x0E, 0x05, 0x1E, 0x04, /* $ */ 0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03, /* % */                  \
        0x0C, 0x12, 0x14, 0x08, 0x15, 0x12, 0x0D, /* & */ 0x0C, 0x04, 0x08, 0x00, 0x00, 0x00, 0x00, /* ' */                  \
        0x02, 0x04, 0x08, 0x08, 0x08, 0x04, 0x02, /* ( */ 0x08, 0x04, 0x02, 0x02, 0x02, 0x04, 0x08, /* ) */                  \
        0x00, 0x04, 0x15, 0x0E, 0x15, 0x04, 0x00, /* * */ 0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00, /* + */                  \
        0x00, 0x00, 0x00, 0x00, 0x0C, 0x04, 0x08, /* , */ 0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00, /* - */                  \
        0x00, 0x00, 0x00, 0x00, 0x00, 0x0E, 0x0E, /* . */ 0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00, /* / */                  \
        0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E, /* 0 */ 0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E, /* 1 */                  \
        0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F, /* 2 */ 0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E, /* 3 */                  \
        0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02, /* 4 */ 0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E, /* 5 */                  \
        0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E, /* 6 */ 0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08, /* 7 */                  \
        0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E, /* 8 */ 0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C, /* 9 */                  \
        0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00, /* : */ 0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x04, 0x08, /* ; */                  \
        0x02, 0x04, 0x08, 0x10, 0x08, 0x04, 0x02, /* < */ 0x00, 0x00, 0x1F, 0x00, 0x1F, 0x00, 0x00, /* = */                  \
        0x08, 0x04, 0x02, 0x01, 0x02, 0x04, 0x08, /* > */ 0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04, /* ? */                  \
        0x0E, 0x11, 0x01, 0x0D, 0x15, 0x15, 0x0E, /* @ */ 0x0E, 0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, /* A */                  \
        0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E, /* B */ 0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E, /* C */                  \
        0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C, /* D */ 0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F, /* E */                  \
        0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10, /* F */ 0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F, /* G */                  \
        0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11, /* H */ 0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E, /* I */                  \
        0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C, /* J */ 0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11, /* K */                  \
        0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F, /* L */ 0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11, /* M */                  \
        0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11, /* N */ 0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E, /* O */                  \
        0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10, /* P */ 0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D, /* Q */                  \
        0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11, /* R */ 0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E, /* S */                  \
        0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04, /* T */ 0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E, /* U */                  \
        0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04, /* V */ 0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A, /* W */                  \
        0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11, /* X */ 0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04, /* Y */                  \
        0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F, /* Z */ 0x0E, 0x08, 0x08, 0x08, 0x08, 0x08, 0x0E, /* [ */                  \
        0x00, 0x10, 0x08, 0x04, 0x02, 0x01, 0x00, /* \ */ 0x0E, 0x02, 0x02, 0x02, 0x02, 0x02, 0x0E, /* ] */                  \
        0x04, 0x0A, 0x11, 0x00, 0x00, 0x00, 0x00, /* ^ */ 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F, /* _ */                  \
        0x08, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00, /* ` */ 0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F, /* a */                  \
        0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E, /* b */ 0x00, 0x00, 0x0E, 0x10, 0x10, 0x11, 0x0E, /* c */                  \
        0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F, /* d */ 0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E, /* e */                  \
        0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08, /* f */ 0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x0E, /* g */                  \
        0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11, /* h */ 0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E, /* i */                  \
        0x02, 0x00, 0x06, 0x02, 0x02, 0x12, 0x0C, /* j */ 0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12, /* k */                  \
        0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E, /* l */ 0x00, 0x00, 0x1A, 0x15, 0x15, 0x11, 0x11, /* m */                  \
        0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11, /* n */ 0x00, 0x00, 0x0E, 0x11, 0x11, 0x11, 0x0E, /* o */                  \
        0x00, 0x00, 0x1E, 0x11, 0x1E, 0x10, 0x10, /* p */ 0x00, 0x00, 0x0D, 0x13, 0x0F, 0x01, 0x01, /* q */                  \
        0x00, 0x00, 0x16, 0x19, 0x10, 0x10, 0x10, /* r */ 0x00, 0x00, 0x0E, 0x10, 0x0E, 0x01, 0x1E, /* s */                  \
        0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06, /* t */ 0x00, 0x00, 0x11, 0x11, 0x11, 0x13, 0x0D, /* u */                  \
        0x00, 0x00, 0x11, 0x11, 0x11, 0x0A, 0x04, /* v */ 0x00, 0x00, 0x11, 0x11, 0x15, 0x15, 0x0A, /* w */                  \
        0x00, 0x00, 0x11, 0x0A, 0x04, 0x0A, 0x11, /* x */ 0x00, 0x00, 0x11, 0x11, 0x0F, 0x01, 0x0E, /* y */                  \
        0x00, 0x00, 0x1F, 0x02, 0x04, 0x08, 0x1F, /* z */ 0x02, 0x04, 0x04, 0x08, 0x04, 0x04, 0x02, /* { */                  \
        0x04, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04, /* | */ 0x08, 0x04, 0x04, 0x02, 0x04, 0x04, 0x08, /* } */                  \
        0x00, 0x00, 0x08, 0x15, 0x02, 0x00, 0x00  /* ~ */                                                                    \
    }

// "#" + 10 digits + " " + FID_LABEL_MAX name bytes + ": " + "9.99" = 50
#define FID_DRAW_TEXT_MAX 52

// one gallery row's label: what the label table holds per row, on the host and on the device
struct fid_draw_label {
    uint8_t name[FID_LABEL_MAX];   // printable ASCII ('?' for every other byte)
    uint8_t len;
    uint8_t bgr[3];
};

// one face of one frame, ready to be tested pixel by pixel.  The thickness and the text scale are the style's: the same for every face.
struct fid_draw_face {
    int32_t ex0, ey0, ex1, ey1;    // the extent of the whole pixel set, clipped to the frame, inclusive; ex0 > ex1: the face draws nothing
    int32_t x1, y1, x2, y2;
    int32_t L;                     // corner length
    int32_t bar_top;               // y2 - bh
    uint8_t bgr[3];
    uint8_t has_bar;
    uint8_t ntext;
    uint8_t pad_[3];
    uint8_t text[FID_DRAW_TEXT_MAX];
};
#define FID_DRAW_FACE_WORDS 25
static_assert(sizeof(fid_draw_face) == 4 * FID_DRAW_FACE_WORDS, "fid_draw_face is copied as 25 dwords");
static_assert(sizeof(fid_draw_label) == FID_LABEL_MAX + 4, "fid_draw_label is copied to the device as 36-byte entries");

FID_HD int fid_draw_imin(int a, int b) { return a < b ? a : b; }
FID_HD int fid_draw_imax(int a, int b) { return a > b ? a : b; }

// the colour of gallery row g when the caller gives none
FID_HD void fid_draw_default_bgr(int g, uint8_t *bgr) {
    const uint32_t h = (uint32_t)(g + 1) * 2654435761u;
    bgr[0] = (uint8_t)(h >> 24); bgr[1] = (uint8_t)((h >> 16) & 255u); bgr[2] = (uint8_t)((h >> 8) & 255u);
}

// label of row g from the caller's name bytes [len] (cut at FID_LABEL_MAX) and colour (NULL: the default)
FID_HD void fid_draw_make_label(fid_draw_label *o, int g, const char *name, int len, const uint8_t *bgr) {
    const int n = fid_draw_imin(fid_draw_imax(len, 0), FID_LABEL_MAX);
    for (int i = 0; i < FID_LABEL_MAX; i++) {
        const uint8_t c = i < n ? (uint8_t)name[i] : (uint8_t)0;
        o->name[i] = i < n ? ((c >= 0x20 && c <= 0x7E) ? c : (uint8_t)'?') : (uint8_t)0;
    }
    o->len = (uint8_t)n;
    if (bgr) { o->bgr[0] = bgr[0]; o->bgr[1] = bgr[1]; o->bgr[2] = bgr[2]; }
    else fid_draw_default_bgr(g, o->bgr);
}

// the similarity as the label shows it: hundredths of s, rounded to nearest, ties to even -- Python's f"{np.float32(s):.2f}": s * 100 is exact
// in double (24 + 7 significant bits)
FID_HD int fid_draw_cents(float s) {
    const double c = rint((double)s * 100.0);
    return c < 999.0 ? (int)c : 999;
}

FID_HD float fid_draw_mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;                  // (one IEEE multiply: nothing to contract with)
#endif
}

// faces of frame b under the three identity forms (include/faceid.h); row0: the first row of the frame in the rows form
FID_HD int fid_draw_face_count(int b, const int32_t *counts, int cap, bool has_idx, int id_stride, const int32_t *offsets, int n_rows, int *row0) {
    *row0 = 0;
    if (has_idx && offsets) {
        const long long lo = offsets[b], hi = offsets[b + 1] < n_rows ? offsets[b + 1] : n_rows;
        long long n = hi - lo;
        if (lo < 0 || n < 0) n = 0;            // (a negative first row names no row at all)
        *row0 = (int)(lo < 0 ? 0 : lo);
        return (int)(n < cap ? n : cap);
    }
    int n = fid_draw_imin(fid_draw_imax(counts[b], 0), cap);
    if (has_idx) n = fid_draw_imin(n, id_stride);
    return n;
}

// The record of one face.  d: its det row (x1, y1, x2, y2, conf); label: the row of the label table for a known face, NULL for an unknown one
// (the caller decides `known` = 0 <= idx < G and a table is there); track_id < 0: none.
FID_HD void fid_draw_make_face(fid_draw_face *o, const float *d, const fid_draw_label *label, float score, int track_id,
                               const fid_draw_style *st, int H, int W) {
    o->ex0 = 1; o->ey0 = 1; o->ex1 = 0; o->ey1 = 0;
    o->x1 = o->y1 = o->x2 = o->y2 = 0; o->L = 0; o->bar_top = 0;
    o->bgr[0] = o->bgr[1] = o->bgr[2] = 0; o->has_bar = 0; o->ntext = 0; o->pad_[0] = o->pad_[1] = o->pad_[2] = 0;
    for (int i = 0; i < FID_DRAW_TEXT_MAX; i++) o->text[i] = 0;
    for (int i = 0; i < 4; i++)
        if (!(fabsf(d[i]) < 8388608.f)) return;                 // NaN, infinity, |v| >= 2^23
    const int x1 = (int)d[0], y1 = (int)d[1], x2 = (int)d[2], y2 = (int)d[3];
    const int w = x2 - x1, h = y2 - y1;
    if (!(w > 0 && h > 0)) return;
    o->x1 = x1; o->y1 = y1; o->x2 = x2; o->y2 = y2;
    o->L = (int)(st->proportion * (double)fid_draw_imin(w, h));
    const uint8_t *c = label ? label->bgr : st->unknown_bgr;
    o->bgr[0] = c[0]; o->bgr[1] = c[1]; o->bgr[2] = c[2];
    const float s = (score > 0.f && score <= 3.4028234663852886e38f) ? score : 0.f;       // finite and positive, else 0
    int n = 0;
    if ((st->flags & FID_DRAW_TRACK_ID) && track_id >= 0) {
        char dig[10];
        int nd = 0, v = track_id;
        do { dig[nd++] = (char)('0' + v % 10); v /= 10; } while (v > 0);
        o->text[n++] = '#';
        while (nd > 0) o->text[n++] = (uint8_t)dig[--nd];
        if (label) o->text[n++] = ' ';
    }
    if (label) {
        for (int i = 0; i < label->len; i++) o->text[n++] = label->name[i];
        const int cents = fid_draw_cents(s);
        o->text[n++] = ':'; o->text[n++] = ' ';
        o->text[n++] = (uint8_t)('0' + cents / 100); o->text[n++] = '.';
        o->text[n++] = (uint8_t)('0' + (cents / 10) % 10); o->text[n++] = (uint8_t)('0' + cents % 10);
    }
    const int t = st->text_scale, r = (st->thickness - 1) / 2;
    o->ntext = (uint8_t)(t > 0 ? n : 0);
    int ex0 = x1 - r, ex1 = x2 + r, ey0 = y1 - r, ey1 = y2 + r;
    if (label && st->bar) {
        // a product of 2^24 or more lifts the bar's top above every row a frame can have: the same pixels as any larger height
        const float p = fid_draw_mul_rn(s, (float)h);
        const int bh = p < 16777216.f ? (int)p : 16777216;
        o->has_bar = 1;
        o->bar_top = y2 - bh;
        ex1 = fid_draw_imax(ex1, x2 + 20);
        ey0 = fid_draw_imin(ey0, o->bar_top);
    }
    if (o->ntext) {
        ex1 = fid_draw_imax(ex1, x1 + 6 * t * o->ntext - 1);
        ey0 = fid_draw_imin(ey0, y1 - 10 - 7 * t + 1);
    }
    ex0 = fid_draw_imax(ex0, 0); ey0 = fid_draw_imax(ey0, 0); ex1 = fid_draw_imin(ex1, W - 1); ey1 = fid_draw_imin(ey1, H - 1);
    if (ex0 > ex1 || ey0 > ey1) return;                         // wholly outside the frame
    o->ex0 = ex0; o->ey0 = ey0; o->ex1 = ex1; o->ey1 = ey1;
}

// is pixel (x, y) in the face's set?  r = (thickness - 1) / 2, t = text scale, font: the 95 x 7 table
FID_HD bool fid_draw_covers(const fid_draw_face *fc, int x, int y, int r, int t, const uint8_t *font) {
    if (x < fc->ex0 || x > fc->ex1 || y < fc->ey0 || y > fc->ey1) return false;
    const int x1 = fc->x1, y1 = fc->y1, x2 = fc->x2, y2 = fc->y2, L = fc->L;
    const bool in_x = x >= x1 && x <= x2, in_y = y >= y1 && y <= y2;
    if (((y == y1 || y == y2) && in_x) || ((x == x1 || x == x2) && in_y)) return true;                       // outline
    // the four horizontal arms lie on rows y1 and y2, the four vertical ones on columns x1 and x2, each grown by r on every side
    const bool near_row = (y >= y1 - r && y <= y1 + r) || (y >= y2 - r && y <= y2 + r);
    const bool near_col = (x >= x1 - r && x <= x1 + r) || (x >= x2 - r && x <= x2 + r);
    if (near_row && ((x >= x1 - r && x <= x1 + L + r) || (x >= x2 - L - r && x <= x2 + r))) return true;
    if (near_col && ((y >= y1 - r && y <= y1 + L + r) || (y >= y2 - L - r && y <= y2 + r))) return true;
    if (fc->has_bar && x >= x2 + 10 && x <= x2 + 20 && y >= fc->bar_top && y <= y2) return true;             // bar
    if (fc->ntext) {
        const int Y = y1 - 10, dx = x - x1, dy = Y - y;        // dy: rows above the cell's bottom row
        if (dx >= 0 && dy >= 0 && dy < 7 * t && dx < 6 * t * fc->ntext) {
            const int k = dx / (6 * t), col = (dx - k * 6 * t) / t, row = 6 - dy / t;
            if (col < 5 && ((font[(fc->text[k] - 0x20) * 7 + row] >> (4 - col)) & 1)) return true;
        }
    }
    return false;
}

// can the rectangle [X0, X1] x [Y0, Y1] hold a pixel of the face's set?  Never false for a rectangle that does (the culls of draw.hip rest
// on that); false for one outside the extent, and for one inside the box's interior -- more than r pixels from all four border lines, where
// neither outline nor arm reaches -- that meets neither the bar's nor the text's rectangle.
FID_HD bool fid_draw_touches(const fid_draw_face *fc, int X0, int Y0, int X1, int Y1, int r, int t) {
    if (X1 < fc->ex0 || X0 > fc->ex1 || Y1 < fc->ey0 || Y0 > fc->ey1) return false;
    const int x1 = fc->x1, y1 = fc->y1, x2 = fc->x2, y2 = fc->y2;
    const bool on_box = X1 >= x1 - r && X0 <= x2 + r && Y1 >= y1 - r && Y0 <= y2 + r;
    const bool interior = X0 > x1 + r && X1 < x2 - r && Y0 > y1 + r && Y1 < y2 - r;
    if (on_box && !interior) return true;
    if (fc->has_bar && X1 >= x2 + 10 && X0 <= x2 + 20 && Y1 >= fc->bar_top && Y0 <= y2) return true;
    if (fc->ntext && X1 >= x1 && X0 <= x1 + 6 * t * fc->ntext - 1 && Y1 >= y1 - 10 - 7 * t + 1 && Y0 <= y1 - 10) return true;
    return false;
}

// argument checks shared by the device and the host entry point; NULL = fine, else what is wrong
inline const char *fid_draw_check(const void *frames, long long B, long long H, long long W, const void *det, const void *counts, long long cap,
                                  const void *idx, const void *score, int id_stride, const void *offsets, int n_rows, const fid_draw_style *st) {
    if (!frames || !det || !counts || !st) return "a NULL frames, det, counts or style pointer";
    if (B <= 0 || H <= 0 || W <= 0 || cap <= 0) return "B, H, W and cap must be positive";
    if (cap > 0x7FFFFFFFll / B || W > 0x7FFFFFFFll / 3 / H) return "B * cap or H * W * 3 overflows int32";
    if (st->thickness < 1 || st->thickness > 15 || st->thickness % 2 == 0) return "thickness must be odd, 1 .. 15";
    if (st->text_scale < 0 || st->text_scale > 4) return "text_scale outside 0 .. 4";
    if (!(st->proportion >= 0.0 && st->proportion <= 1.0)) return "proportion NaN or outside [0, 1]";
    if (idx && !score) return "idx without score";
    if (idx && !offsets && id_stride <= 0) return "id_stride must be positive in the slot form";
    if (n_rows < 0) return "n_rows is negative";
    return nullptr;
}
