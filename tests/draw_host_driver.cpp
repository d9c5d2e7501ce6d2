// Stand-alone host program around csrc/draw_core.h (tests/test_draw_host_sanitized.py builds it with -fsanitize=address,undefined and runs it):
// reads one drawing case from a file, rasterises every frame into a heap buffer of exactly H * W * 3 bytes with the header's record and
// coverage functions, and writes the frames out.  Every input array is a heap allocation of exactly its size, too.
//
// input:  int32 B, H, W, cap, G, thickness, text_scale, bar; float64 proportion; float32 det [B,cap,5]; int32 counts [B]; int32 idx [B,cap];
//         float32 score [B,cap]; int32 name_offsets [G+1]; the name bytes.  Slots form (id_stride = cap), default colours, frames start black.
// output: uint8 [B,H,W,3]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "draw_core.h"

static const uint8_t font[FID_DRAW_GLYPHS * 7] = FID_DRAW_FONT_INIT;

template <typename T>
static T *read_array(FILE *f, size_t n) {
    T *p = (T *)malloc(n * sizeof(T) + (n == 0));
    if (!p || fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t *hd = read_array<int32_t>(f, 8);
    const int B = hd[0], H = hd[1], W = hd[2], cap = hd[3], G = hd[4];
    fid_draw_style st;
    memset(&st, 0, sizeof(st));
    st.thickness = hd[5]; st.text_scale = hd[6]; st.bar = hd[7];
    st.unknown_bgr[0] = 255;
    double *prop = read_array<double>(f, 1);
    st.proportion = *prop;
    float *det = read_array<float>(f, (size_t)B * cap * 5);
    int32_t *counts = read_array<int32_t>(f, B);
    int32_t *idx = read_array<int32_t>(f, (size_t)B * cap);
    float *score = read_array<float>(f, (size_t)B * cap);
    int32_t *off = read_array<int32_t>(f, (size_t)G + 1);
    char *names = read_array<char>(f, (size_t)off[G]);
    fclose(f);
    const char *why = fid_draw_check(det, B, H, W, det, counts, cap, idx, score, cap, nullptr, 0, &st);
    if (why) { fprintf(stderr, "%s\n", why); return 3; }
    fid_draw_label *tab = (fid_draw_label *)malloc((size_t)G * sizeof(fid_draw_label) + (G == 0));
    for (int g = 0; g < G; g++) fid_draw_make_label(&tab[g], g, names + off[g], off[g + 1] - off[g], nullptr);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int r = (st.thickness - 1) / 2, t = st.text_scale;
    long lit = 0;
    for (int b = 0; b < B; b++) {
        uint8_t *img = (uint8_t *)calloc((size_t)H * W * 3, 1);      // exactly one frame: a pixel outside it is a heap overflow
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, true, cap, nullptr, 0, &row0);
        for (int k = 0; k < n; k++) {
            const size_t slot = (size_t)b * cap + k;
            const bool known = idx[slot] >= 0 && idx[slot] < G;
            fid_draw_face fc;
            fid_draw_make_face(&fc, det + slot * 5, known ? &tab[idx[slot]] : nullptr, score[slot], -1, &st, H, W);
            // the culls of the device kernels: a 64 x 16 tile or a strip of four pixels that fid_draw_touches rules out holds no pixel of the set
            for (int cw = 64, ch = 16, pass = 0; pass < 2; pass++, cw = 4, ch = 1)
                for (int y0 = 0; y0 < H; y0 += ch)
                    for (int x0 = 0; x0 < W; x0 += cw) {
                        const int xe = x0 + cw - 1 < W - 1 ? x0 + cw - 1 : W - 1, ye = y0 + ch - 1 < H - 1 ? y0 + ch - 1 : H - 1;
                        if (fid_draw_touches(&fc, x0, y0, xe, ye, r, t)) continue;
                        for (int y = y0; y <= ye; y++)
                            for (int x = x0; x <= xe; x++)
                                if (fid_draw_covers(&fc, x, y, r, t, font)) { fprintf(stderr, "face %d of frame %d: culled pixel (%d, %d)\n", k, b, x, y); return 4; }
                    }
            for (int y = fc.ey0; y <= fc.ey1; y++)
                for (int x = fc.ex0; x <= fc.ex1; x++)
                    if (fid_draw_covers(&fc, x, y, r, t, font)) {
                        uint8_t *p = img + ((size_t)y * W + x) * 3;
                        p[0] = fc.bgr[0]; p[1] = fc.bgr[1]; p[2] = fc.bgr[2];
                        lit++;
                    }
        }
        fwrite(img, 1, (size_t)H * W * 3, o);
        free(img);
    }
    fclose(o);
    free(tab); free(names); free(off); free(score); free(idx); free(counts); free(det); free(prop); free(hd);
    printf("%ld\n", lit);
    return 0;
}
