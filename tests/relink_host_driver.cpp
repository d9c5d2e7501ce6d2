// Stand-alone host program around csrc/relink_core.h (tests/test_relink_host_sanitized.py builds it with -fsanitize=address,undefined and runs
// it): reads a relinker's shape and the tables of consecutive steps from a file, runs the header's walk over each step from the fresh state
// and writes the person table and the state after every step.  Every array is a heap allocation of exactly its size: a read past a frame's
// last detection, past the last row or the last pool entry, or a write past a table's last word ends the program.
//
// input:  int32 S, T, L, dim, B, cap, calls, window, max_age; float32 thresh; then per call: int32 row_cap, n_rows, stream [B], counts [B],
//         track [B,cap,2], offsets [B+1], src [row_cap], fp16 q [n_rows,dim]
// output: per call: int32 person [B,cap,2], live [S,T,8], pool [S,L,8], frames [S], fp16 live_q [S,T,dim], pool_q [S,L,dim]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "relink_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 9);
    float *thresh = read_array<float>(f, 1);
    const int S = hd[0], T = hd[1], L = hd[2], dim = hd[3], B = hd[4], cap = hd[5], calls = hd[6];
    if (!fid_relink_shape_ok(S, T, L, dim) || B < 1 || cap < 1 || calls < 0) { fprintf(stderr, "bad header\n"); return 2; }
    fid_relink_config cfg;
    cfg.thresh = thresh[0]; cfg.window = hd[7]; cfg.max_age = hd[8];
    const size_t nl = (size_t)S * T, np = (size_t)S * L, faces = (size_t)B * cap;
    int32_t *live = new_array<int32_t>(nl * FID_RELINK_WORDS), *pool = new_array<int32_t>(np * FID_RELINK_WORDS), *frames = new_array<int32_t>((size_t)S);
    uint16_t *live_q = new_array<uint16_t>(nl * dim), *pool_q = new_array<uint16_t>(np * dim);
    fid_relink_state_clear(live, live_q, pool, pool_q, frames, S, T, L, dim, -1);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    int rc = 0;
    for (int call = 0; call < calls && rc == 0; call++) {
        int32_t *sz = read_array<int32_t>(f, 2);
        const int row_cap = sz[0], n_rows = sz[1];
        if (row_cap < 1 || n_rows < 0) { fprintf(stderr, "bad sizes\n"); return 2; }
        int32_t *stream = read_array<int32_t>(f, (size_t)B);
        int32_t *counts = read_array<int32_t>(f, (size_t)B);
        int32_t *track = read_array<int32_t>(f, faces * 2);
        int32_t *offsets = read_array<int32_t>(f, (size_t)B + 1);
        int32_t *src = read_array<int32_t>(f, (size_t)row_cap);
        uint16_t *q = read_array<uint16_t>(f, (size_t)n_rows * dim);
        int32_t *person = new_array<int32_t>(faces * 2);
        const char *why = fid_relink_check(S, T, L, dim, stream, B, cap, counts, track, offsets, src, row_cap, n_rows, q, &cfg, person);
        if (why) {
            fprintf(stderr, "refused: %s\n", why);
            rc = 3;
        } else {
            fid_track_relink_table_host(live, live_q, pool, pool_q, frames, S, T, L, dim, stream, B, cap, counts, track, offsets, src, row_cap,
                                        n_rows, q, &cfg, person);
            fwrite(person, sizeof(int32_t), faces * 2, o);
            fwrite(live, sizeof(int32_t), nl * FID_RELINK_WORDS, o);
            fwrite(pool, sizeof(int32_t), np * FID_RELINK_WORDS, o);
            fwrite(frames, sizeof(int32_t), (size_t)S, o);
            fwrite(live_q, sizeof(uint16_t), nl * dim, o);
            fwrite(pool_q, sizeof(uint16_t), np * dim, o);
        }
        free(person); free(q); free(src); free(offsets); free(track); free(counts); free(stream); free(sz);
    }
    fclose(o);
    fclose(f);
    if (rc == 0) printf("%d\n", calls);
    free(pool_q); free(live_q); free(frames); free(pool); free(live); free(thresh); free(hd);
    return rc;
}
