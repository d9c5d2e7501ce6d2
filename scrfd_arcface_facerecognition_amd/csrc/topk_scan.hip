// Fused top-k gallery search: the k best rows per query for any k <= FID_TOPK_MAX, without the n x G score matrix.
//
// reference qdrant_manager.py:138-183 (`search_similar(limit, score_threshold)`), smart_face_recognition.py:1619-1643 (search_person, limit 5) and
// :2618-2652 (is_duplicate_image, limit 1): `limit` is an arbitrary integer.  fid_gallery_topk writes the whole score matrix per chunk of queries
// and serves five values of k; here the GEMM of fid_match keeps, per query, a short sorted list of packed keys in registers instead.
//
//   key     = sortable(score) << 32 | ~(first_row + row), the key of fid_match_keys: unsigned order = score descending, lowest row first, and
//             keys of different rows differ -- so "the K largest keys" is one well-defined set whatever order the scores are seen in.  Score <= 0
//             and NaN give no key (0); queries >= n and rows >= G read as zeros (buffer bounds), score 0.
//   tile    = range_join.hip's: 128 queries x 128 gallery rows, four waves of 4 x 4 mfma_f32_16x16x32_f16 fragments, register-staged buffer loads
//             into an XOR-swizzled LDS double buffer, one __syncthreads() per K-step, no hand-counted waits (a private copy of the loop: the
//             epilogue below reuses the staging LDS, which the shared tile code does not foresee).
//   slice   = a workgroup owns one query tile and `tps` consecutive gallery tiles and carries its lists across them; S slices give n_qt x S
//             workgroups (about two per CU; FID_TOPK_SLICES forces S).  Workgroups of one slice are neighbours: they share its gallery tiles in L2.
//   select  = after a tile's K-loop the 32 KB of staging are free: the sums go through them in two passes of 64 gallery rows (waves wn = pass
//             write theirs, 16-byte stores, [row][query] with the 4-query groups XOR-ed by the row so that neither the 8-lane groups of the
//             stores nor the 32-lane groups of the loads collide).  Thread t owns query t & 127 and rows 32 (t >> 7) .. + 31 of each pass: it
//             reads four sums, and only if their maximum reaches the score of its K-th key does it build keys and insert (a statically indexed
//             compare-and-swap chain; the list never leaves the registers).
//   merge   = every (query, slice, thread half) list goes to the scratch arena once, with plain vector stores; topk_merge (one wave per query)
//             lets each lane keep the best K of its share, then k rounds of wave maximum.  No atomics: the answer does not depend on S or on
//             which workgroup finishes first.  The same kernel merges the [parts, n, k] keys of row shards (fid_topk_merge).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "topk_keys.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int TT = 128, TCK = 32;                         // tile edge (both operands), K-step
constexpr int TMI = 4, TNI = 4;                           // fragments of a wave: 64 queries x 64 gallery rows
constexpr int TOP_BYTES = TT * TCK * 2;                   // 8 KB per operand and step
constexpr unsigned TOOB = 0xFFFFFF00u;                    // past every operand (both are checked to be smaller)
constexpr size_t CAND_BYTES_MAX = 256ull << 20;           // what fid_gallery_topk allows its score matrix

struct TSArgs {
    const void *q, *g;
    u64 *cand;                                            // [n][S][2][KP]
    int n, G, dim, n_qt, n_gt, tps, S, col0;
    unsigned q_bytes, g_bytes;
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 k, int m) {
    return ((u64)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), m) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, m);
}

template <int KP>
__global__ void __launch_bounds__(256) topk_scan(const TSArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TOP_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int qt = (int)(blockIdx.x % (unsigned)a.n_qt), sl = (int)(blockIdx.x / (unsigned)a.n_qt);
    const int gt_end = min(sl * a.tps + a.tps, a.n_gt);

    const auto rs_q = __builtin_amdgcn_make_buffer_rsrc((void *)a.q, 0, a.q_bytes, 0x00020000);
    const auto rs_g = __builtin_amdgcn_make_buffer_rsrc((void *)a.g, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    // per K-step a thread stages two 16-byte pieces of each operand: rows lrow and lrow + 64, group lgrp
    const int lrow = tid >> 2, lgrp = tid & 3;
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);      // (row + 64: the same swizzle)
    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = TOP_BYTES + (wn * 64 + frow) * 64 + grp;
    const int ksteps = a.dim / TCK;

    unsigned q_off[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int qr = qt * TT + lrow + 64 * i;
        q_off[i] = qr < a.n ? (unsigned)qr * rowb + (unsigned)lgrp * 16u : TOOB;
    }

    // this thread's list: query myq of the tile, gallery rows 32 half .. + 31 of every 64-row pass
    const int myq = tid & 127, half = tid >> 7;
    u64 best[KP];
#pragma unroll
    for (int j = 0; j < KP; j++) best[j] = 0ull;
    float floor_s = 0.f;                                    // the score of best[KP - 1] (0 while the list is not full)
    float *sc = (float *)smem;                              // the pass buffer: [64 rows][128 queries] fp32 = the 32 KB of staging

    for (int gt = sl * a.tps; gt < gt_end; gt++) {
        unsigned g_off[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int gr = gt * TT + lrow + 64 * i;
            g_off[i] = gr < a.G ? (unsigned)gr * rowb + (unsigned)lgrp * 16u : TOOB;
        }
        u32x4 rq[2], rg[2];
        auto issue_loads = [&](int ks) {
            const unsigned kb = (unsigned)ks * (TCK * 2);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                rq[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_q, q_off[i] != TOOB ? q_off[i] + kb : TOOB, 0, 0);
                rg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_g, g_off[i] != TOOB ? g_off[i] + kb : TOOB, 0, 0);
            }
        };
        auto store_tiles = [&](int buf) {
            char *dst = smem + buf * 2 * TOP_BYTES + st_off;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                *(u32x4 *)(dst + i * 64 * 64) = rq[i];
                *(u32x4 *)(dst + TOP_BYTES + i * 64 * 64) = rg[i];
            }
        };

        f32x4 acc[TMI][TNI];
#pragma unroll
        for (int mi = 0; mi < TMI; mi++)
#pragma unroll
            for (int ni = 0; ni < TNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

        issue_loads(0);
        store_tiles(0);                                     // (the pass buffer of the tile before was last read behind a barrier)
        __syncthreads();
        for (int ks = 0; ks < ksteps; ks++) {
            const int cur = ks & 1;
            const bool more = ks + 1 < ksteps;
            if (more) issue_loads(ks + 1);
            const char *st = smem + cur * 2 * TOP_BYTES;
            half8 qf[TMI], gf[TNI];
#pragma unroll
            for (int mi = 0; mi < TMI; mi++) qf[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
            for (int ni = 0; ni < TNI; ni++) gf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
            for (int mi = 0; mi < TMI; mi++)
#pragma unroll
                for (int ni = 0; ni < TNI; ni++)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[mi], gf[ni], acc[mi][ni], 0, 0, 0);
            if (more) store_tiles(cur ^ 1);                 // last read in step ks - 1, behind that step's barrier
            __syncthreads();
        }

        // ---- select: acc[mi][ni][j] = query (64 wm + 16 mi + 4 (lane >> 4) + j) x gallery row (64 wn + 16 ni + (lane & 15)) of the tile ----
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
            if (wn == pass) {
#pragma unroll
                for (int mi = 0; mi < TMI; mi++)
#pragma unroll
                    for (int ni = 0; ni < TNI; ni++) {
                        const int r = ni * 16 + (lane & 15), qg = wm * 16 + mi * 4 + (lane >> 4);
                        *(f32x4 *)(sc + r * TT + ((qg ^ (r & 31)) << 2)) = acc[mi][ni];
                    }
            }
            __syncthreads();
            const int row0 = a.col0 + gt * TT + pass * 64;
#pragma unroll 1
            for (int r = half * 32; r < half * 32 + 32; r += 4) {
                float s[4];
#pragma unroll
                for (int e = 0; e < 4; e++) s[e] = sc[(r + e) * TT + (((myq >> 2) ^ ((r + e) & 31)) << 2) + (myq & 3)];
                const float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));   // (fmaxf drops a NaN; four NaNs fail the comparison)
                if (m >= floor_s && m > 0.f) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (s[e] >= floor_s && s[e] > 0.f) {
                            const u64 key = make_key(s[e], row0 + r + e);
                            if (key > best[KP - 1]) {                   // (equal scores: the lower row has the larger key)
                                list_insert<KP>(best, key);
                                floor_s = best[KP - 1] ? key_score(best[KP - 1]) : 0.f;
                            }
                        }
                    }
                }
            }
            __syncthreads();                                // the buffer is free for the next pass / the next tile's first K-step
        }
    }

    const int q = qt * TT + myq;
    if (q < a.n) {
        ulonglong2 *dst = (ulonglong2 *)(a.cand + (((size_t)q * a.S + sl) * 2 + half) * KP);
#pragma unroll
        for (int j = 0; j < KP; j += 2) dst[j >> 1] = make_ulonglong2(best[j], best[j + 1]);
    }
}

// one wave per query: the k largest of its parts x count keys, descending.  Keys that are 0 or name a row >= G_total are no candidates.
// keys_out != NULL: the keys themselves ([n, k], 0 behind the last); otherwise (idx, score) under the strict threshold, (-1, 0.0) behind the last hit.
template <int KP>
__global__ void __launch_bounds__(256) topk_merge(const u64 *__restrict__ keys, int parts, long long stride_p, long long stride_q, int count, int n,
                                                  int k, int G_total, float thresh, u64 *__restrict__ keys_out, int *__restrict__ idx_out,
                                                  float *__restrict__ score_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    u64 best[KP];
#pragma unroll
    for (int j = 0; j < KP; j++) best[j] = 0ull;
    for (int p = 0; p < parts; p++) {
        const u64 *src = keys + (size_t)p * stride_p + (size_t)row * stride_q;
        for (int i = lane; i < count; i += 64) {
            const u64 key = src[i];
            const int j = (int)(~(unsigned)key);
            if (key != 0ull && j >= 0 && j < G_total && key > best[KP - 1]) list_insert<KP>(best, key);
        }
    }
    const float floor_ = thresh > 0.f ? thresh : 0.f;
    for (int t = 0; t < k; t++) {
        u64 w = best[0];                                    // every lane's list is descending: its head is its candidate
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = shfl_xor_u64(w, o);
            w = other > w ? other : w;
        }
        if (w != 0ull && best[0] == w) {                    // the winning lane advances
#pragma unroll
            for (int j = 0; j + 1 < KP; j++) best[j] = best[j + 1];
            best[KP - 1] = 0ull;
        }
        if (lane == 0) {
            if (keys_out) {
                keys_out[(size_t)row * k + t] = w;
            } else {
                const float s = key_score(w);
                const bool ok = w != 0ull && s > floor_;
                idx_out[(size_t)row * k + t] = ok ? (int)(~(unsigned)w) : -1;
                score_out[(size_t)row * k + t] = ok ? s : 0.f;
            }
        }
    }
}

}  // namespace

void launch_merge(fid_ctx *ctx, const u64 *keys, int parts, long long stride_p, long long stride_q, int count, int n, int k, int G_total,
                  float thresh, u64 *keys_out, int32_t *idx, float *score) {
#define MERGE(KK) hipLaunchKernelGGL(topk_merge<KK>, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, keys, parts, stride_p, stride_q, count, n, k, \
                                     G_total, thresh, keys_out, idx, score)
    switch (list_len(k)) { case 8: MERGE(8); break; case 16: MERGE(16); break; default: MERGE(32); }
#undef MERGE
}

namespace {

// the scan + the merge of its lists into keys [n, k] (the context's mutex is held).  keys_out == NULL: the keys go to the front of the scratch
// arena and *keys_arena names them (fid_gallery_search: they never leave the device's scratch).
int scan_keys(fid_ctx *ctx, fid_gallery *g, const void *q, int n, int k, int first_row, u64 *keys_out, u64 **keys_arena) {
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    FID_REQUIRE(dim > 0 && dim % TCK == 0, "top-k: embedding dim %d must be a multiple of %d", dim, TCK);
    const int KP = list_len(k);
    const int n_gt = cdiv(G, TT);
    // slices: about two workgroups per CU; with one query tile all the parallelism is here.  Never more slices than gallery tiles, and
    // never so many that one query tile's lists pass the arena's limit.  FID_TOPK_SLICES (read per call) forces S: tests, measurements
    long long S = std::max(1, 2 * ctx->num_cus / cdiv(n, TT));
    if (const char *e = getenv("FID_TOPK_SLICES")) S = std::max(1, atoi(e));
    const size_t list_bytes = (size_t)2 * KP * 8;           // per query and slice
    S = std::min<long long>({S, (long long)n_gt, (long long)(CAND_BYTES_MAX / (TT * list_bytes))});
    const int tps = cdiv(n_gt, (int)S);
    S = cdiv(n_gt, tps);                                    // no empty slice
    long long chunk = std::min<long long>(n, (long long)(CAND_BYTES_MAX / (S * list_bytes)) / TT * TT);
    chunk = std::min<long long>(chunk, (long long)(0xFFFFFF00ull / ((size_t)dim * 2)) / TT * TT - TT);
    FID_REQUIRE(chunk > 0 && (size_t)Gp * dim * 2 + (size_t)TT * dim * 2 < 0xFFFFFF00ull, "top-k: operand larger than 4 GiB");
    const size_t keys_bytes = keys_out ? 0 : (((size_t)n * k * 8 + 255) & ~(size_t)255);
    void *ws;
    FID_TRY(get_scratch(ctx, 3, keys_bytes + (size_t)chunk * S * list_bytes, &ws));
    if (!keys_out) keys_out = *keys_arena = (u64 *)ws;
    TSArgs a{};
    a.g = rows; a.G = G; a.dim = dim; a.col0 = first_row;
    a.cand = (u64 *)((char *)ws + keys_bytes);
    a.n_gt = n_gt; a.tps = tps; a.S = (int)S;
    a.g_bytes = (unsigned)((size_t)Gp * dim * 2);
    for (long long q0 = 0; q0 < n; q0 += chunk) {
        const int m = (int)std::min<long long>(chunk, n - q0);
        a.q = (const char *)q + (size_t)q0 * dim * 2;
        a.n = m;
        a.n_qt = cdiv(m, TT);
        a.q_bytes = (unsigned)((size_t)m * dim * 2);
        const dim3 grid((unsigned)(a.n_qt * a.S));
        switch (KP) {
            case 8: hipLaunchKernelGGL(topk_scan<8>, grid, dim3(256), 0, ctx->stream, a); break;
            case 16: hipLaunchKernelGGL(topk_scan<16>, grid, dim3(256), 0, ctx->stream, a); break;
            default: hipLaunchKernelGGL(topk_scan<32>, grid, dim3(256), 0, ctx->stream, a); break;
        }
        const int count = (int)(S * 2 * KP);
        launch_merge(ctx, a.cand, 1, 0, count, count, m, k, 0x7FFFFFFF, 0.f, keys_out + (size_t)q0 * k, nullptr, nullptr);
    }
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // namespace
}  // namespace fid

extern "C" {

int fid_topk_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, int first_row, uint64_t *keys_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && keys_dev, "top-k keys: NULL context, gallery, query or output pointer");
    FID_REQUIRE(n > 0, "top-k keys: %d queries", n);
    FID_REQUIRE(k >= 1 && k <= FID_TOPK_MAX, "top-k keys: k = %d is outside 1 .. %d", k, FID_TOPK_MAX);
    int Gp = 0;
    FID_TRY(fid_gallery_info(g, nullptr, &Gp, nullptr));
    FID_REQUIRE(first_row >= 0 && (long long)first_row + Gp < 0x7FFFFFFFll, "top-k keys: global gallery index overflows 31 bits");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    return scan_keys(ctx, g, query_f16_dev, n, k, first_row, (u64 *)keys_dev, nullptr);
}

int fid_topk_merge(fid_ctx *ctx, const uint64_t *keys_dev, int parts, int n, int k, int G_total, float thresh, int32_t *idx_dev,
                   float *score_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && keys_dev && idx_dev && score_dev, "top-k merge: NULL context, key or output pointer");
    FID_REQUIRE(parts > 0 && n > 0 && G_total > 0, "top-k merge: parts %d, queries %d, rows %d must be positive", parts, n, G_total);
    FID_REQUIRE(k >= 1 && k <= FID_TOPK_MAX, "top-k merge: k = %d is outside 1 .. %d", k, FID_TOPK_MAX);
    FID_REQUIRE(!std::isnan(thresh), "top-k merge: the threshold is NaN");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    launch_merge(ctx, (const u64 *)keys_dev, parts, (long long)n * k, k, k, n, k, G_total, thresh, nullptr, idx_dev, score_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// exactly fid_topk_keys(first_row = 0) followed by fid_topk_merge(parts = 1): one code path for the sharded and the unsharded search
int fid_gallery_search(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, float thresh, int32_t *idx_dev,
                       float *score_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && idx_dev && score_dev, "search: NULL context, gallery, query or output pointer");
    FID_REQUIRE(n > 0, "search: %d queries", n);
    FID_REQUIRE(k >= 1 && k <= FID_TOPK_MAX, "search: k = %d is outside 1 .. %d (fid_gallery_range serves every hit above a threshold)", k, FID_TOPK_MAX);
    FID_REQUIRE(!std::isnan(thresh), "search: the threshold is NaN");
    int G = 0, Gp = 0;
    FID_TRY(fid_gallery_info(g, &G, &Gp, nullptr));
    FID_REQUIRE((long long)Gp < 0x7FFFFFFFll, "search: global gallery index overflows 31 bits");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    u64 *keys = nullptr;
    FID_TRY(scan_keys(ctx, g, query_f16_dev, n, k, 0, nullptr, &keys));
    launch_merge(ctx, keys, 1, (long long)n * k, k, k, n, k, G, thresh, nullptr, idx_dev, score_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // extern "C"
