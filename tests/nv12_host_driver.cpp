// Stand-alone host program around csrc/yuv_core.h (tests/test_nv12_cpu.py builds it with -fsanitize=address,undefined and runs it): reads one
// NV12 batch and its layout from a file, checks the layout and converts the frames with the header's functions, and writes the BGR frames
// out.  The batch is a heap allocation of exactly the size the file states: a read past the last UV row of the last frame ends the program.
//
// input:  int32 B, H, W, pitch, standard; int64 uv_offset, frame_stride, n_bytes; uint8 nv12 [n_bytes]
// output: uint8 bgr [B,H,W,3]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "yuv_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 5);
    int64_t *ld = read_array<int64_t>(f, 3);
    const int B = hd[0], H = hd[1], W = hd[2];
    fid_nv12_desc d;
    memset(&d, 0, sizeof d);
    d.pitch = hd[3]; d.standard = hd[4]; d.uv_offset = ld[0]; d.frame_stride = ld[1];
    if (ld[2] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    uint8_t *nv12 = read_array<uint8_t>(f, (size_t)ld[2]);
    fclose(f);
    int rc = 0;
    const char *why = fid_nv12_check(&d, B, H, W);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        rc = 3;
    } else {
        const size_t n = (size_t)B * H * W * 3;
        uint8_t *bgr = (uint8_t *)malloc(n);
        fid_nv12_to_bgr_frames_host(nv12, &d, B, H, W, bgr);
        FILE *o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        fwrite(bgr, 1, n, o);
        fclose(o);
        printf("%zu\n", n);
        free(bgr);
    }
    free(nv12); free(ld); free(hd);
    return rc;
}
