// Stand-alone host program around csrc/measure_core.h (tests/test_measure_host_sanitized.py builds it with -fsanitize=address,undefined and runs
// it): reads one table of crops from a file, measures every row with the header's functions and writes the 16 words per row out.  Every array is
// a heap allocation of exactly its size: a read before row 15 / column 15 of a crop's window neighbourhood, past a crop, past the landmark
// table or the matrices, or a signed overflow in the sums ends the program.
//
// input:  int32 n_rows, n_kps, has_src, has_pose; uint8 crops [n_rows,112,112,3]; int32 src [n_rows] (if has_src); float32 kps [n_kps,10] and
//         float64 M [n_rows,6] (if has_pose)
// output: int64 stats [n_rows,8]; float32 measure [n_rows,8]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "measure_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 4);
    const int n = hd[0], n_kps = hd[1], has_src = hd[2], has_pose = hd[3];
    if (n < 0 || n_kps < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t crop_bytes = (size_t)FID_MEASURE_CROP * FID_MEASURE_CROP * 3;
    int32_t *src = nullptr;
    float *kps = nullptr;
    double *M = nullptr;
    // one allocation per crop: a read past a crop's end lands in a red zone, not in its neighbour
    uint8_t **crop = (uint8_t **)malloc(sizeof(uint8_t *) * n + (n == 0));
    for (int i = 0; i < n; i++) crop[i] = read_array<uint8_t>(f, crop_bytes);
    if (has_src) src = read_array<int32_t>(f, n);
    if (has_pose) { kps = read_array<float>(f, (size_t)n_kps * 10); M = read_array<double>(f, (size_t)n * 6); }
    fclose(f);
    int64_t *stats = (int64_t *)malloc(sizeof(int64_t) * 8 * n + (n == 0));
    float *measure = (float *)malloc(sizeof(float) * 8 * n + (n == 0));
    for (int i = 0; i < n; i++) {
        if (src && src[i] >= n_kps) { fprintf(stderr, "row %d: src %d outside the landmark table\n", i, src[i]); return 3; }
        if (!src && kps && i >= n_kps) { fprintf(stderr, "row %d: no landmark row\n", i); return 3; }
        // row i alone through the table loop: its own crop allocation, its src entry (without a table: landmark row i), its M row, its output words
        fid_measure_table_host(crop[i], 1, kps ? kps + (src ? 0 : (size_t)i * 10) : nullptr, src ? src + i : nullptr, M ? M + (size_t)i * 6 : nullptr,
                               stats + (size_t)i * 8, measure + (size_t)i * 8);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(stats, sizeof(int64_t), (size_t)n * 8, o);
    fwrite(measure, sizeof(float), (size_t)n * 8, o);
    fclose(o);
    for (int i = 0; i < n; i++) free(crop[i]);
    free(crop); free(measure); free(stats); free(M); free(kps); free(src); free(hd);
    printf("%d\n", n);
    return 0;
}
