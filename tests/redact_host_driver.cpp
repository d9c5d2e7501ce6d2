// Stand-alone host program around csrc/redact_core.h (tests/test_redact_host_sanitized.py builds it with -fsanitize=address,undefined and runs
// it): reads one redaction case from a file, redacts its frames in a heap buffer of exactly B * H * W * 3 bytes -- or of exactly n_bytes, the
// NV12 allocation, which the test lets end with the last UV byte of the last frame -- with the header's host loops, and writes the buffer
// out.  Every input array is a heap allocation of exactly its size, too: a byte read or written outside a frame, a read past an input or a
// signed overflow in the geometry ends the program.
//
// input:  int32 B, H, W, cap, mode, who, cells, nv12, pitch, standard, solid, fill b, g, r; int64 uv_offset, frame_stride, n_bytes;
//         float64 expand; float32 det [B,cap,5]; int32 counts [B]; int32 idx [B,cap]; uint8 frames [n_bytes] (absent when solid >= 0: every
//         byte is `solid`).  Slots form (id_stride = cap).
// output: uint8 [n_bytes]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "redact_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 14);
    int64_t *ld = read_array<int64_t>(f, 3);
    const int B = hd[0], H = hd[1], W = hd[2], cap = hd[3], nv12 = hd[7], solid = hd[10];
    fid_redact_style st;
    memset(&st, 0, sizeof(st));
    st.mode = hd[4]; st.who = hd[5]; st.cells = hd[6];
    st.fill_bgr[0] = (uint8_t)hd[11]; st.fill_bgr[1] = (uint8_t)hd[12]; st.fill_bgr[2] = (uint8_t)hd[13];
    fid_nv12_desc d;
    memset(&d, 0, sizeof d);
    d.pitch = hd[8]; d.standard = hd[9]; d.uv_offset = ld[0]; d.frame_stride = ld[1];
    if (ld[2] < 0 || B <= 0 || cap <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t n_bytes = (size_t)ld[2];
    double *ex = read_array<double>(f, 1);
    st.expand = *ex;
    float *det = read_array<float>(f, (size_t)B * cap * 5);
    int32_t *counts = read_array<int32_t>(f, B);
    int32_t *idx = read_array<int32_t>(f, (size_t)B * cap);
    float *score = (float *)calloc((size_t)B * cap, sizeof(float));
    uint8_t *frames;
    if (solid >= 0) {
        frames = (uint8_t *)malloc(n_bytes + (n_bytes == 0));
        if (!frames) { fprintf(stderr, "out of memory\n"); return 2; }
        memset(frames, solid, n_bytes);
    } else {
        frames = read_array<uint8_t>(f, n_bytes);
    }
    fclose(f);
    const char *why = fid_redact_check(frames, B, H, W, det, counts, cap, idx, score, cap, nullptr, 0, &st);
    if (!why && nv12) why = fid_nv12_check(&d, B, H, W);
    if (!why && !nv12 && n_bytes != (size_t)B * H * W * 3) why = "n_bytes is not B * H * W * 3";
    if (why) { fprintf(stderr, "refused: %s\n", why); return 3; }
    const bool ok = nv12 ? fid_redact_frames_nv12_host(frames, &d, B, H, W, det, counts, cap, idx, cap, nullptr, 0, &st)
                         : fid_redact_frames_host(frames, B, H, W, det, counts, cap, idx, cap, nullptr, 0, &st);
    if (!ok) { fprintf(stderr, "out of memory\n"); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(frames, 1, n_bytes, o);
    fclose(o);
    free(frames); free(score); free(idx); free(counts); free(det); free(ex); free(ld); free(hd);
    return 0;
}
