// Stand-alone host program around csrc/calib_core.h (tests/test_calib_host_sanitized.py builds it with -fsanitize=address,undefined and runs
// it): reads one score-distribution case from a file, runs the header's loops and writes the six outputs.  Every array is a heap allocation of
// exactly its size: a read past the last gallery row, position or label, or a write past an output's last entry, ends the program.
//
// input:  int32 G, dim, n, has_rows, bins; fp16 rows [G,dim]; with has_rows, int32 rows [n]; int32 labels [n]
// output: uint64 hist [2][bins]; int32 imp_via [n]; float32 imp_score [n]; int32 gen_via [n]; float32 gen_score [n]; uint64 summary [4]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "calib_core.h"

template <typename T>
static T *read_array(FILE *f, size_t n) {
    T *p = (T *)malloc(n * sizeof(T) + (n == 0));
    if (!p || fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return p;
}

template <typename T>
static T *new_array(size_t n) {
    T *p = (T *)malloc(n * sizeof(T) + (n == 0));
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0x5A, n * sizeof(T));
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t *hd = read_array<int32_t>(f, 5);
    const int G = hd[0], dim = hd[1], n = hd[2], has_rows = hd[3], bins = hd[4];
    if (G < 1 || dim < 1 || n < 1 || (!has_rows && n != G)) { fprintf(stderr, "bad header\n"); return 2; }
    uint16_t *g = read_array<uint16_t>(f, (size_t)G * dim);
    int32_t *rows = has_rows ? read_array<int32_t>(f, (size_t)n) : nullptr;
    int32_t *labels = read_array<int32_t>(f, (size_t)n);
    fclose(f);
    const size_t hn = bins > 0 ? (size_t)2 * bins : 0;
    uint64_t *hist = new_array<uint64_t>(hn), *summary = new_array<uint64_t>(FID_HIST_SUMMARY_WORDS);
    int32_t *imp_via = new_array<int32_t>((size_t)n), *gen_via = new_array<int32_t>((size_t)n);
    float *imp_score = new_array<float>((size_t)n), *gen_score = new_array<float>((size_t)n);
    int rc = 0;
    const char *why = fid_score_hist_check(g, G, dim, labels, n, bins, hist, imp_via, imp_score, gen_via, gen_score, summary);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        rc = 3;
    } else {
        fid_score_hist_table_host(g, G, dim, rows, labels, n, bins, hist, imp_via, imp_score, gen_via, gen_score, summary);
        FILE *o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        fwrite(hist, sizeof(uint64_t), hn, o);
        fwrite(imp_via, sizeof(int32_t), (size_t)n, o);
        fwrite(imp_score, sizeof(float), (size_t)n, o);
        fwrite(gen_via, sizeof(int32_t), (size_t)n, o);
        fwrite(gen_score, sizeof(float), (size_t)n, o);
        fwrite(summary, sizeof(uint64_t), FID_HIST_SUMMARY_WORDS, o);
        fclose(o);
        printf("%d\n", n);
    }
    free(gen_score); free(imp_score); free(gen_via); free(imp_via); free(summary); free(hist);
    free(labels); free(rows); free(g); free(hd);
    return rc;
}
