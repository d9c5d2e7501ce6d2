// Stand-alone host program around csrc/cluster_core.h (tests/test_cluster_host_sanitized.py builds it with -fsanitize=address,undefined and
// runs it): reads one clustering case from a file, runs the header's walk and writes the five outputs.  Every array is a heap allocation of
// exactly its size: a read past the last gallery row or the last position, or a write past an output's last entry, ends the program.
//
// input:  int32 G, dim, n, has_rows, min_pts; float32 thresh; fp16 rows [G,dim]; with has_rows, int32 rows [n]
// output: int32 label [n], degree [n], via [n]; float32 score [n]; int32 summary [6]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cluster_core.h"

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
    float *thresh = read_array<float>(f, 1);
    const int G = hd[0], dim = hd[1], n = hd[2], has_rows = hd[3], min_pts = hd[4];
    if (G < 1 || dim < 1 || n < 1 || (!has_rows && n != G)) { fprintf(stderr, "bad header\n"); return 2; }
    uint16_t *g = read_array<uint16_t>(f, (size_t)G * dim);
    int32_t *rows = has_rows ? read_array<int32_t>(f, (size_t)n) : nullptr;
    fclose(f);
    int32_t *label = new_array<int32_t>((size_t)n), *degree = new_array<int32_t>((size_t)n), *via = new_array<int32_t>((size_t)n);
    float *score = new_array<float>((size_t)n);
    int32_t *summary = new_array<int32_t>(FID_CLUSTER_SUMMARY_WORDS);
    int rc = 0;
    const char *why = fid_cluster_check(g, G, dim, n, thresh[0], min_pts, label, degree, via, score, summary);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        rc = 3;
    } else {
        fid_cluster_table_host(g, G, dim, rows, n, thresh[0], min_pts, label, degree, via, score, summary);
        FILE *o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        fwrite(label, sizeof(int32_t), (size_t)n, o);
        fwrite(degree, sizeof(int32_t), (size_t)n, o);
        fwrite(via, sizeof(int32_t), (size_t)n, o);
        fwrite(score, sizeof(float), (size_t)n, o);
        fwrite(summary, sizeof(int32_t), FID_CLUSTER_SUMMARY_WORDS, o);
        fclose(o);
        printf("%d\n", n);
    }
    free(summary); free(score); free(via); free(degree); free(label);
    free(rows); free(g); free(thresh); free(hd);
    return rc;
}
