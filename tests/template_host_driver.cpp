// Stand-alone host program around csrc/template_core.h (tests/test_template_host_sanitized.py builds it with -fsanitize=address,undefined and
// runs it): reads one identity-template case from a file, runs the header's loops and writes the six outputs.  Every array is a heap
// allocation of exactly its size: a read past the last gallery row, position, label or weight, or a write past an output's last entry, ends
// the program.
//
// input:  int32 G, dim, n, has_rows, has_weights, P; float32 min_score; fp16 rows [G,dim]; with has_rows, int32 rows [n]; int32 labels [n];
//         with has_weights, int32 weights [n]
// output: fp16 templates [P,dim]; float32 score [n]; int32 kept [n]; int32 person [P,4]; float32 cohesion [P]; int64 summary [6]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "template_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 6);
    float *ms = read_array<float>(f, 1);
    const int G = hd[0], dim = hd[1], n = hd[2], has_rows = hd[3], has_weights = hd[4], P = hd[5];
    const float min_score = ms[0];
    if (G < 1 || dim < 1 || n < 1 || (!has_rows && n != G)) { fprintf(stderr, "bad header\n"); return 2; }
    uint16_t *g = read_array<uint16_t>(f, (size_t)G * dim);
    int32_t *rows = has_rows ? read_array<int32_t>(f, (size_t)n) : nullptr;
    int32_t *labels = read_array<int32_t>(f, (size_t)n);
    int32_t *weights = has_weights ? read_array<int32_t>(f, (size_t)n) : nullptr;
    fclose(f);
    const size_t Pn = P > 0 ? (size_t)P : 0;
    uint16_t *tpl = new_array<uint16_t>(Pn * dim);
    float *score = new_array<float>((size_t)n), *cohesion = new_array<float>(Pn);
    int32_t *kept = new_array<int32_t>((size_t)n), *person = new_array<int32_t>(Pn * 4);
    int64_t *summary = new_array<int64_t>(FID_TEMPLATE_SUMMARY_WORDS);
    int rc = 0;
    const char *why = fid_templates_check(g, G, dim, labels, n, P, min_score, tpl, score, kept, person, cohesion, summary);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        rc = 3;
    } else {
        fid_templates_table_host(g, G, dim, rows, labels, weights, n, P, min_score, tpl, score, kept, person, cohesion, summary);
        FILE *o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        fwrite(tpl, sizeof(uint16_t), Pn * dim, o);
        fwrite(score, sizeof(float), (size_t)n, o);
        fwrite(kept, sizeof(int32_t), (size_t)n, o);
        fwrite(person, sizeof(int32_t), Pn * 4, o);
        fwrite(cohesion, sizeof(float), Pn, o);
        fwrite(summary, sizeof(int64_t), FID_TEMPLATE_SUMMARY_WORDS, o);
        fclose(o);
        printf("%d\n", n);
    }
    free(summary); free(person); free(kept); free(cohesion); free(score); free(tpl);
    free(weights); free(labels); free(rows); free(g); free(ms); free(hd);
    return rc;
}
