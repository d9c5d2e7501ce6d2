// Merging duplicate persons of the store, in id order: the reference's find_and_merge_duplicates loop as one asynchronous call.
//
// reference smart_face_recognition.py:2755-2792 walks its persons in ascending id; a person whose embedding is gone is skipped (:2757-2759) and
// every person still alive absorbs each alive LARGER id its range search returns at >= merge_duplicate_threshold (:2774 skips self and smaller
// ids).  Over the positions k = 0 .. n - 1 of the ids in ascending order that is
//
//     keeper[k] = the LOWEST position j < k with keeper[j] == -1 and hit(j, k), else -1          ("first alive", not "best score")
//
// with hit = the rule of fid_gallery_range (range_join.hip): fp32 cosine of the two stored fp16 rows >= thresh and > 0.  The walk is sequential
// only in WHO IS STILL ALIVE; the cosines are not.  The chain of visit_group.hip resolves it, positions cut into blocks of 128:
//
//   prepare        one wave per position: alive[k] = "the row is inside the gallery and has a non-zero element" (the sign bit does not count:
//                  the -0.0 marker row of an empty slot is a zero row).  Such a position TAKES PART; any other never hits and is never hit.
//   dedup_cross    (block b, grid = b) the 128 x 128 tile of block b against block c < b (the tile code of range_join.hip / visit_group.hip:
//                  mfma_f32_16x16x32_f16, register-staged buffer loads into a plain LDS double buffer, one __syncthreads() per K-step, no
//                  hand-counted waits; the operand rows are read THROUGH rows[]: nothing is gathered, no scratch copy of the rows exists).
//                  Epilogue: per query the minimum key position << 32 | score bits over the columns that survived and hit (a hit score is > 0,
//                  so its bits carry it as they are; one tile alone computes a given pair, so the score of a position is unique), a 16-lane
//                  reduction and one 64-bit atomicMin per query and wave.  A block without a survivor is skipped.
//   dedup_resolve  (block b, ONE workgroup) the block's own cosines by the same tile code into LDS, then wave 0 walks the 128 positions in
//                  order.  A cross result always precedes an in-block candidate (its position is lower); otherwise lane l holds "survived"
//                  for the candidates l and l + 64 and two ballots name the lowest one that hits.  One wave, state in registers, no barrier
//                  inside the walk.  All threads then write keeper / score / alive of the block.
//   dedup_apply    (apply != 0) one wave per position: an absorbed position's gallery row is set to +0.0 with plain 16-byte vector stores.
//
// Launch chain on the context's stream: prepare, resolve(0), cross(1), resolve(1), cross(2), resolve(2) ... apply.  Order between blocks comes
// ONLY from stream order: no workgroup waits for another one, no flag is polled, nothing is launched cooperatively.  Any dependency depth is
// therefore exact (a path of 300 alternates survive / absorbed 150 levels deep).  No n x n or n x G matrix and no pair list exists anywhere.
#include <cmath>

#include "common.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int DT = 128, DCK = 32;                         // block of positions = tile edge, K-step
constexpr int DMI = 4, DNI = 4;                           // fragments of a wave: 64 x 64
constexpr int DOP_BYTES = DT * DCK * 2;                   // 8 KB per operand and step
constexpr unsigned DOOB = 0xFFFFFF00u;                    // past the gallery (checked to be smaller): such a load returns zeros
constexpr unsigned long long NO_KEY = ~0ull;
constexpr int DS_LD = 144;                                // floats per row of the block's cosine matrix in LDS (visit_group.hip)
constexpr int OFF_S = 2 * 2 * DOP_BYTES;                  // [128][144] fp32
constexpr int OFF_KEY = OFF_S + DT * DS_LD * 4;           // [128] keys of dedup_cross
constexpr int OFF_NZ = OFF_KEY + DT * 8;                  // [128] in: the position takes part; out: it takes part and survived
constexpr int OFF_KEEP = OFF_NZ + DT * 4;                 // [128] keeper
constexpr int OFF_SCORE = OFF_KEEP + DT * 4;              // [128] score
constexpr int RESOLVE_LDS = OFF_SCORE + DT * 4;           // 109 056 bytes

struct DDArgs {
    void *gal;                                            // [Gp][dim] unit fp16
    const int32_t *rows;                                  // [n] gallery row of every position
    unsigned long long *keys;                             // [n]
    int32_t *alive, *blk_alive, *state;                   // [n], [blocks] survivors per block, {absorbed, took part} so far
    int32_t *keeper, *summary;
    float *score;
    float thresh;
    int n, G, dim;
    unsigned g_bytes;
};

__device__ __forceinline__ bool is_hit(float s, float thresh) { return s >= thresh && s > 0.f; }      // (a NaN fails both)

// positions pos_a .. + 127 x positions pos_b .. + 127 (a position >= n or with a row outside the gallery reads as zeros):
// acc[mi][ni][j] = position (pos_a + 64 wm + 16 mi + 4 (lane >> 4) + j) x position (pos_b + 64 wn + 16 ni + (lane & 15)).  Ends behind a barrier.
__device__ __forceinline__ void tile_gemm(const DDArgs &a, int pos_a, int pos_b, char *smem, int tid, int lane, int wm, int wn,
                                          f32x4 (&acc)[DMI][DNI]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.gal, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    const int lrow = tid >> 2, lgrp = tid & 3;
    unsigned a_src[2], b_src[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pa = pos_a + lrow + 64 * i, pb = pos_b + lrow + 64 * i;
        const int ra = pa < a.n ? a.rows[pa] : -1, rb = pb < a.n ? a.rows[pb] : -1;
        a_src[i] = (ra >= 0 && ra < a.G) ? (unsigned)ra * rowb + (unsigned)lgrp * 16u : DOOB;
        b_src[i] = (rb >= 0 && rb < a.G) ? (unsigned)rb * rowb + (unsigned)lgrp * 16u : DOOB;
    }
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);
    u32x4 ra[2], rb[2];
    auto issue_loads = [&](int ks) {
        const unsigned kb = (unsigned)ks * (DCK * 2);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, a_src[i] != DOOB ? a_src[i] + kb : DOOB, 0, 0);
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_src[i] != DOOB ? b_src[i] + kb : DOOB, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
        char *dst = smem + buf * 2 * DOP_BYTES + st_off;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(u32x4 *)(dst + i * 64 * 64) = ra[i];
            *(u32x4 *)(dst + DOP_BYTES + i * 64 * 64) = rb[i];
        }
    };
#pragma unroll
    for (int mi = 0; mi < DMI; mi++)
#pragma unroll
        for (int ni = 0; ni < DNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = a.dim / DCK;
    issue_loads(0);
    store_tiles(0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = DOP_BYTES + (wn * 64 + frow) * 64 + grp;
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;
        if (more) issue_loads(ks + 1);
        const char *st = smem + cur * 2 * DOP_BYTES;
        half8 af[DMI], bf[DNI];
#pragma unroll
        for (int mi = 0; mi < DMI; mi++) af[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
        for (int ni = 0; ni < DNI; ni++) bf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
        for (int mi = 0; mi < DMI; mi++)
#pragma unroll
            for (int ni = 0; ni < DNI; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        if (more) store_tiles(cur ^ 1);                     // last read in step ks - 1, behind that step's barrier
        __syncthreads();
    }
}

// one wave per position: does it take part?  Also resets the per-call state.
__global__ void __launch_bounds__(256) dedup_prepare(const DDArgs a, int n_blocks) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < n_blocks) a.blk_alive[gid] = 0;
    if (gid == 0) { a.state[0] = 0; a.state[1] = 0; }
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pos >= a.n) return;
    const int row = a.rows[pos];
    unsigned any = 0;
    if (row >= 0 && row < a.G) {                            // (wave-uniform)
        const unsigned *r = (const unsigned *)((const char *)a.gal + (size_t)row * a.dim * 2);
        for (int i = lane; i < a.dim / 2; i += 64) any |= r[i] & 0x7FFF7FFFu;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= (unsigned)__shfl_xor((int)any, o);
    if (lane == 0) a.alive[pos] = any != 0u;
}

// block b (queries) x block c = blockIdx.x < b (candidates)
__global__ void __launch_bounds__(256) dedup_cross(const DDArgs a, int b) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * DOP_BYTES];
    const int c = blockIdx.x;
    if (a.blk_alive[c] == 0) return;                        // (block-uniform, before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    f32x4 acc[DMI][DNI];
    tile_gemm(a, b * DT, c * DT, smem, tid, lane, wm, wn, acc);
    const int q0 = b * DT + wm * 64 + (lane >> 4) * 4, c0 = c * DT + wn * 64 + (lane & 15);
    int al[DNI];
#pragma unroll
    for (int ni = 0; ni < DNI; ni++) al[ni] = a.alive[c0 + ni * 16];            // (c < b: every column is a position < n, decided already)
#pragma unroll
    for (int mi = 0; mi < DMI; mi++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned long long key = NO_KEY;
#pragma unroll
            for (int ni = DNI - 1; ni >= 0; ni--)           // (descending: the lowest column that hits is assigned last)
                if (al[ni] && is_hit(acc[mi][ni][j], a.thresh))
                    key = ((unsigned long long)(unsigned)(c0 + ni * 16) << 32) | __float_as_uint(acc[mi][ni][j]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const unsigned long long k = ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(key >> 32), o) << 32) |
                                             (unsigned)__shfl_xor((int)(unsigned)key, o);
                key = k < key ? k : key;
            }
            const int qi = q0 + mi * 16 + j;
            if ((lane & 15) == 0 && qi < a.n && key != NO_KEY) atomicMin(a.keys + qi, key);
        }
}

// block b, one workgroup
__global__ void __launch_bounds__(256) dedup_resolve(const DDArgs a, int b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int base = b * DT, m = min(DT, a.n - base);
    float *S = (float *)(smem + OFF_S);
    unsigned long long *keyl = (unsigned long long *)(smem + OFF_KEY);
    int *nzl = (int *)(smem + OFF_NZ), *keepl = (int *)(smem + OFF_KEEP);
    float *scorel = (float *)(smem + OFF_SCORE);
    if (tid < DT) {
        keyl[tid] = tid < m ? a.keys[base + tid] : NO_KEY;
        nzl[tid] = tid < m ? a.alive[base + tid] : 0;
    }
    {
        f32x4 acc[DMI][DNI];
        tile_gemm(a, base, base, smem, tid, lane, wm, wn, acc);
        const int r0 = wm * 64 + (lane >> 4) * 4, c0 = wn * 64 + (lane & 15);
#pragma unroll
        for (int mi = 0; mi < DMI; mi++)
#pragma unroll
            for (int ni = 0; ni < DNI; ni++)
#pragma unroll
                for (int j = 0; j < 4; j++) S[(r0 + mi * 16 + j) * DS_LD + c0 + ni * 16] = acc[mi][ni][j];
    }
    __syncthreads();
    if (wave == 0) {
        // every lane holds the same counters; lane l alone holds "survived" of the candidates l and l + 64
        int absorbed = 0, part = 0, survivors = 0;
        int s0 = 0, s1 = 0;
        for (int i = 0; i < m; i++) {
            const unsigned long long key = keyl[i];
            int keep = -1;
            float score = 0.f;
            if (key != NO_KEY) {                            // (wave-uniform) an earlier block's survivor: a lower position than any in this block
                keep = (int)(unsigned)(key >> 32);
                score = __uint_as_float((unsigned)key);
            } else if (survivors > 0) {                     // (wave-uniform)
                const bool h0 = lane < i && s0 && is_hit(S[i * DS_LD + lane], a.thresh);
                const bool h1 = lane + 64 < i && s1 && is_hit(S[i * DS_LD + 64 + lane], a.thresh);
                const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
                const int j = m0 ? __ffsll((long long)m0) - 1 : (m1 ? 64 + __ffsll((long long)m1) - 1 : -1);
                if (j >= 0) { keep = base + j; score = S[i * DS_LD + j]; }
            }
            const int nz = nzl[i];                          // (a position that takes no part has cosine 0 with everything: keep is -1)
            const int surv = nz && keep < 0;
            part += nz; absorbed += keep >= 0; survivors += surv;
            if (lane == (i & 63)) { if (i < 64) s0 = surv; else s1 = surv; }
            if (lane == 0) { keepl[i] = keep; scorel[i] = score; nzl[i] = surv; }
        }
        if (lane == 0) {
            const int tot_abs = a.state[0] + absorbed, tot_part = a.state[1] + part;
            a.state[0] = tot_abs; a.state[1] = tot_part; a.blk_alive[b] = survivors;
            if (base + m >= a.n) { a.summary[0] = tot_abs; a.summary[1] = tot_part; }
        }
    }
    __syncthreads();
    if (tid < m) { a.keeper[base + tid] = keepl[tid]; a.score[base + tid] = scorel[tid]; a.alive[base + tid] = nzl[tid]; }
}

// one wave per position: the row of an absorbed position becomes the row fid_gallery_set_rows leaves for a zero embedding
__global__ void __launch_bounds__(256) dedup_apply(const DDArgs a) {
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pos >= a.n || a.keeper[pos] < 0) return;
    const int row = a.rows[pos];
    if (row < 0 || row >= a.G) return;                      // (an absorbed position took part, so its row is inside; kept as the bounds check)
    uint4 *dst = (uint4 *)((char *)a.gal + (size_t)row * a.dim * 2);
    for (int k = lane; k < a.dim / 8; k += 64) dst[k] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace
}  // namespace fid

extern "C" int fid_gallery_dedup(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, int n, float thresh, int apply, int32_t *keeper_dev,
                                 float *score_dev, int32_t *summary_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && rows_dev && keeper_dev && score_dev && summary_dev, "dedup: NULL context, gallery, rows or output pointer");
    FID_REQUIRE(n > 0 && n <= FID_DEDUP_MAX_ROWS, "dedup: %d rows (1 .. %d per call)", n, FID_DEDUP_MAX_ROWS);
    FID_REQUIRE(!std::isnan(thresh), "dedup: the threshold is NaN");
    FID_REQUIRE(thresh > 0.f, "dedup: threshold %g must be > 0 (a hit needs a score > 0)", thresh);
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    FID_REQUIRE(dim > 0 && dim % DCK == 0, "dedup: embedding dim %d must be a multiple of %d", dim, DCK);
    FID_REQUIRE((size_t)Gp * dim * 2 + (size_t)DT * dim * 2 < 0xFFFFFF00ull, "dedup: gallery larger than 4 GiB");
    const int n_blocks = cdiv(n, DT);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // scratch slot 2 (fid_match's key array and fid_gallery_group's state; calls are serialised by the context's mutex and ordered by its stream):
    // 12 bytes per position + 4 per block, laid out for n rounded up to 65 536 so that the arena is replaced (behind a stream synchronise, the
    // rule of get_scratch) at most when a call crosses such a step
    const size_t ncap = ((size_t)n + 65535) & ~(size_t)65535;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_alive = up(ncap * 8), o_blk = o_alive + up(ncap * 4), o_state = o_blk + up((ncap / DT) * 4), total = o_state + 256;
    void *ws;
    FID_TRY(get_scratch(ctx, 2, total, &ws));
    DDArgs a{};
    a.gal = rows; a.rows = rows_dev;
    a.keys = (unsigned long long *)ws;
    a.alive = (int32_t *)((char *)ws + o_alive);
    a.blk_alive = (int32_t *)((char *)ws + o_blk);
    a.state = (int32_t *)((char *)ws + o_state);
    a.keeper = keeper_dev; a.score = score_dev; a.summary = summary_dev;
    a.thresh = thresh;
    a.n = n; a.G = G; a.dim = dim;
    a.g_bytes = (unsigned)((size_t)Gp * dim * 2);
    FID_TRY(ensure_dyn_lds(ctx, (const void *)dedup_resolve, RESOLVE_LDS));
    FID_HIP(hipMemsetAsync(a.keys, 0xFF, (size_t)n * 8, ctx->stream));
    hipLaunchKernelGGL(dedup_prepare, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a, n_blocks);
    for (int b = 0; b < n_blocks; b++) {
        if (b > 0) hipLaunchKernelGGL(dedup_cross, dim3(b), dim3(256), 0, ctx->stream, a, b);
        hipLaunchKernelGGL(dedup_resolve, dim3(1), dim3(256), RESOLVE_LDS, ctx->stream, a, b);
    }
    if (apply) hipLaunchKernelGGL(dedup_apply, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}
