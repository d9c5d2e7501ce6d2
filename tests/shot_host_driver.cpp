// Stand-alone host program around csrc/shot_core.h (tests/test_shot_host_sanitized.py builds it with -fsanitize=address,undefined and runs it):
// reads one table of fid_face_measure rows from a file, scores every row with the header's functions and writes the scores out.  Every array is
// a heap allocation of exactly its size: a read past the stats or measure words of the last row, or a write past the scores, ends the program.
//
// input:  int32 n_rows; float32 n_s, n_c, n_r; int64 stats [n_rows,8]; float32 measure [n_rows,8]
// output: float32 score [n_rows]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "shot_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 1);
    float *norms = read_array<float>(f, 3);
    const int n = hd[0];
    if (n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    int64_t *stats = read_array<int64_t>(f, (size_t)n * 8);
    float *measure = read_array<float>(f, (size_t)n * 8);
    fclose(f);
    fid_measure_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.sharpness_normalization = norms[0]; cfg.contrast_normalization = norms[1]; cfg.residual_normalization = norms[2];
    float *score = (float *)malloc(sizeof(float) * n + (n == 0));
    const char *why = fid_shot_score_check(stats, measure, n, &cfg, score);
    int rc = 0;
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        rc = 3;
    } else {
        fid_shot_score_table_host(stats, measure, n, &cfg, score);
        FILE *o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        fwrite(score, sizeof(float), (size_t)n, o);
        fclose(o);
        printf("%d\n", n);
    }
    free(score); free(measure); free(stats); free(norms); free(hd);
    return rc;
}
