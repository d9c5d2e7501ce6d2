// Stand-alone host program around csrc/coast_core.h (tests/test_coast_host_sanitized.py builds it with -fsanitize=address,undefined and runs
// it): reads a coaster's state and the tables of consecutive steps from a file, runs the header's walk over each step and writes the
// outputs and the state after every step.  Every array is a heap allocation of exactly its size: a read past a frame's last detection, a
// write past an output's last filler or past the state's last word ends the program.
//
// input:  int32 S, T, B, cap, calls, hold, predict, has_ident; float32 grow; int32 entries [S,T,16]; then per call: int32 stream [B],
//         float32 det [B,cap,5], int32 counts [B], int32 track [B,cap,2] and, with has_ident, int32 ident_idx [B,cap], float32 ident_score [B,cap]
// output: per call: float32 det_out [B,cap2,5], int32 counts_out [B], int32 track_out [B,cap2,2], int32 idx_out [B,cap2],
//         float32 score_out [B,cap2], int32 entries [S,T,16]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "coast_core.h"

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
    int32_t *hd = read_array<int32_t>(f, 8);
    float *grow = read_array<float>(f, 1);
    const int S = hd[0], T = hd[1], B = hd[2], cap = hd[3], calls = hd[4], has_ident = hd[7];
    if (S < 1 || T < 1 || B < 1 || cap < 1 || calls < 0) { fprintf(stderr, "bad header\n"); return 2; }
    fid_coast_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.hold = hd[5]; cfg.predict = hd[6]; cfg.grow = grow[0];
    const size_t n_entries = (size_t)S * T * FID_COAST_WORDS, faces = (size_t)B * cap, faces2 = (size_t)B * ((size_t)cap + T);
    int32_t *entries = read_array<int32_t>(f, n_entries);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    int rc = 0;
    for (int call = 0; call < calls && rc == 0; call++) {
        int32_t *stream = read_array<int32_t>(f, (size_t)B);
        float *det = read_array<float>(f, faces * 5);
        int32_t *counts = read_array<int32_t>(f, (size_t)B);
        int32_t *track = read_array<int32_t>(f, faces * 2);
        int32_t *ii = has_ident ? read_array<int32_t>(f, faces) : nullptr;
        float *sc = has_ident ? read_array<float>(f, faces) : nullptr;
        float *det_out = new_array<float>(faces2 * 5);
        int32_t *counts_out = new_array<int32_t>((size_t)B);
        int32_t *track_out = new_array<int32_t>(faces2 * 2);
        int32_t *idx_out = new_array<int32_t>(faces2);
        float *score_out = new_array<float>(faces2);
        const char *why = fid_coast_check(S, T, stream, B, cap, det, counts, track, ii, sc, &cfg, det_out, counts_out, track_out, idx_out, score_out);
        if (why) {
            fprintf(stderr, "refused: %s\n", why);
            rc = 3;
        } else {
            fid_track_coast_table_host(entries, S, T, stream, B, cap, det, counts, track, ii, sc, &cfg, det_out, counts_out, track_out, idx_out,
                                       score_out);
            fwrite(det_out, sizeof(float), faces2 * 5, o);
            fwrite(counts_out, sizeof(int32_t), (size_t)B, o);
            fwrite(track_out, sizeof(int32_t), faces2 * 2, o);
            fwrite(idx_out, sizeof(int32_t), faces2, o);
            fwrite(score_out, sizeof(float), faces2, o);
            fwrite(entries, sizeof(int32_t), n_entries, o);
        }
        free(score_out); free(idx_out); free(track_out); free(counts_out); free(det_out);
        free(sc); free(ii); free(track); free(counts); free(det); free(stream);
    }
    fclose(o);
    fclose(f);
    if (rc == 0) printf("%d\n", calls);
    free(entries); free(grow); free(hd);
    return rc;
}
