// Stand-alone host program around csrc/yuv_core.h and csrc/draw_nv12_core.h (tests/test_draw_nv12_cpu.py builds it with
// -fsanitize=address,undefined and runs it): reads one case from a file, converts its BGR frames to NV12 with fid_bgr_to_nv12_frames_host
// and draws its faces onto its NV12 frames with fid_draw_face_nv12_host, and writes both batches out.  Either batch is a heap allocation of
// exactly n_bytes -- the test lets it end with the last UV byte of the last frame --, every input array one of exactly its size: a byte
// written behind a frame, or read past an input, ends the program.
//
// input:  int32 B, H, W, cap, G, thickness, text_scale, bar, pitch, standard; int64 uv_offset, frame_stride, n_bytes; float64 proportion;
//         float32 det [B,cap,5]; int32 counts [B]; int32 idx [B,cap]; float32 score [B,cap]; int32 name_offsets [G+1]; the name bytes;
//         uint8 nv12 [n_bytes] (the frames to draw on); uint8 bgr [B,H,W,3] (the frames to convert).  Slots form, default colours.
// output: uint8 [n_bytes] the drawn frames; uint8 [n_bytes] the converted frames, over a fill of 0xA5
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "draw_nv12_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 10);
    int64_t *ld = read_array<int64_t>(f, 3);
    const int B = hd[0], H = hd[1], W = hd[2], cap = hd[3], G = hd[4];
    fid_draw_style st;
    memset(&st, 0, sizeof(st));
    st.thickness = hd[5]; st.text_scale = hd[6]; st.bar = hd[7];
    st.unknown_bgr[0] = 255;
    fid_nv12_desc d;
    memset(&d, 0, sizeof d);
    d.pitch = hd[8]; d.standard = hd[9]; d.uv_offset = ld[0]; d.frame_stride = ld[1];
    if (ld[2] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t n_bytes = (size_t)ld[2];
    double *prop = read_array<double>(f, 1);
    st.proportion = *prop;
    float *det = read_array<float>(f, (size_t)B * cap * 5);
    int32_t *counts = read_array<int32_t>(f, B);
    int32_t *idx = read_array<int32_t>(f, (size_t)B * cap);
    float *score = read_array<float>(f, (size_t)B * cap);
    int32_t *off = read_array<int32_t>(f, (size_t)G + 1);
    char *names = read_array<char>(f, (size_t)off[G]);
    uint8_t *nv12 = read_array<uint8_t>(f, n_bytes);
    uint8_t *bgr = read_array<uint8_t>(f, (size_t)B * H * W * 3);
    fclose(f);
    const char *why = fid_draw_check(nv12, B, H, W, det, counts, cap, idx, score, cap, nullptr, 0, &st);
    if (!why) why = fid_nv12_check(&d, B, H, W);
    fid_yuv_fwd k;
    if (!why && !fid_yuv_fwd_for(d.standard, &k)) why = "an unknown standard";
    if (why) { fprintf(stderr, "refused: %s\n", why); return 3; }
    fid_draw_label *tab = (fid_draw_label *)malloc((size_t)G * sizeof(fid_draw_label) + (G == 0));
    for (int g = 0; g < G; g++) fid_draw_make_label(&tab[g], g, names + off[g], off[g + 1] - off[g], nullptr);
    const int r = (st.thickness - 1) / 2, t = st.text_scale;
    long lit = 0;
    for (int b = 0; b < B; b++) {
        int row0;
        const int n = fid_draw_face_count(b, counts, cap, true, cap, nullptr, 0, &row0);
        uint8_t *yp = nv12 + (size_t)b * (size_t)d.frame_stride;
        for (int j = 0; j < n; j++) {
            const size_t slot = (size_t)b * cap + j;
            const bool known = idx[slot] >= 0 && idx[slot] < G;
            fid_draw_face fc;
            fid_draw_make_face(&fc, det + slot * 5, known ? &tab[idx[slot]] : nullptr, score[slot], -1, &st, H, W);
            lit += fid_draw_face_nv12_host(&fc, k, yp, yp + d.uv_offset, d.pitch, r, t, font);
        }
    }
    uint8_t *conv = (uint8_t *)malloc(n_bytes + (n_bytes == 0));
    memset(conv, 0xA5, n_bytes);
    fid_bgr_to_nv12_frames_host(bgr, B, H, W, conv, &d);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(nv12, 1, n_bytes, o);
    fwrite(conv, 1, n_bytes, o);
    fclose(o);
    free(conv); free(tab); free(bgr); free(nv12); free(names); free(off); free(score); free(idx); free(counts); free(det); free(prop);
    free(ld); free(hd);
    printf("%ld\n", lit);
    return 0;
}
