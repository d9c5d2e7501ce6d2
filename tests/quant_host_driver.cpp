// Stand-alone host program around csrc/quant_core.h (tests/test_coarse_cpu.py builds it with -fsanitize=address,undefined and runs it): reads a
// table of fp16 rows from a file, quantises every row with the header's functions and writes codes and exponents out.  Every row, its codes and
// its exponent are heap allocations of exactly their sizes: a read past a row, a write past its codes, or a shift or conversion that overflows
// ends the program.
//
// input:  int32 n, dim; uint16 rows [n, dim]
// output: int8 codes [n, dim]; int8 exps [n]
#include <cstdio>
#include <cstdlib>

#include "quant_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 2);
    const int n = hd[0], dim = hd[1];
    if (n < 0 || dim <= 0 || dim > FID_QUANT_DIM_MAX) { fprintf(stderr, "bad header\n"); return 2; }
    // one allocation per row, per code row and per exponent: an access past one lands in a red zone, not in its neighbour
    uint16_t **row = (uint16_t **)malloc(sizeof(uint16_t *) * n + (n == 0));
    int8_t **codes = (int8_t **)malloc(sizeof(int8_t *) * n + (n == 0));
    int8_t **exps = (int8_t **)malloc(sizeof(int8_t *) * n + (n == 0));
    for (int i = 0; i < n; i++) {
        row[i] = read_array<uint16_t>(f, (size_t)dim);
        codes[i] = (int8_t *)malloc((size_t)dim);
        exps[i] = (int8_t *)malloc(1);
        if (!codes[i] || !exps[i]) return 2;
    }
    fclose(f);
    for (int i = 0; i < n; i++) fid_quantize_rows_i8_table_host(row[i], 1, dim, codes[i], exps[i]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    for (int i = 0; i < n; i++) fwrite(codes[i], 1, (size_t)dim, o);
    for (int i = 0; i < n; i++) fwrite(exps[i], 1, 1, o);
    fclose(o);
    for (int i = 0; i < n; i++) { free(row[i]); free(codes[i]); free(exps[i]); }
    free(row); free(codes); free(exps); free(hd);
    printf("%d\n", n);
    return 0;
}
