// Range search / similarity join on the gallery: every (query, gallery row) whose cosine reaches a threshold, not the best k.
//
// reference smart_face_recognition.py:2761-2766 asks its vector store for ALL persons above merge_duplicate_threshold
// (`search_similar(k=len(persons), threshold=...)`, qdrant_manager.py:137-183): a range search.  The arithmetic is the GEMM of fid_match;
// the epilogue keeps what passes the threshold instead of an arg-max, so the n x G score matrix is never written and only the hit
// records leave the device.
//
//   tile    = 128 queries x 128 gallery rows, four waves, wave (wm, wn) = queries 64 wm .. + 63 x gallery rows 64 wn .. + 63
//             (4 x 4 fragments of mfma_f32_16x16x32_f16, 64 fp32 sums per lane)
//   stream  = K-steps of 32 columns, both operands register-staged (buffer loads: rows past the operand read as zeros) into a plain
//             LDS double buffer, one __syncthreads() per step; rows are 64 bytes with the 16-byte groups XOR-swizzled as in
//             match_gemm.hip, so a fragment read (16 rows x 4 groups) is conflict-free.  No hand-counted waits.
//   hit     = score >= thresh && score > 0: `>=` is Qdrant's score_threshold; `> 0` keeps deleted / free rows (all zeros) out whatever
//             the threshold; a NaN fails both comparisons.  Columns >= G and queries >= n are never emitted.
//   compact = every lane counts its hits, a wave prefix sum places them, ONE atomicAdd per wave on a 64-bit counter reserves the slots;
//             records go out with ordinary vector stores, only to slots < hit_cap.  The counter is not clipped: overflow shows after
//             the fact (as with fid_scrfd_check).  Record order depends on which wave adds first; the set and the scores do not (each
//             score is summed in one fixed order).
//   self    = the queries are the gallery's own rows: only tile pairs with gallery tile >= query tile are computed (the linear id walks
//             the upper triangle) and only row > query is emitted, so every unordered pair appears once as (i, j), i < j, and (i, i) never.
//   order   = the linear id walks SUPER-tiles of 16 x 16 tile pairs (the triangle of them in self mode; the lower half of a diagonal
//             super-tile is skipped at once): the 256 pairs that run together read 32 operand tiles, not 257.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int RT = 128, RCK = 32;                         // tile edge (both operands), K-step
constexpr int RMI = 4, RNI = 4;                           // fragments of a wave: 64 queries x 64 gallery rows
constexpr int ROP_BYTES = RT * RCK * 2;                   // 8 KB per operand and step
constexpr unsigned ROOB = 0xFFFFFF00u;                    // past every operand (both are checked to be smaller)

struct RJArgs {
    const void *q, *g;
    int32_t *pairs;
    float *scores;
    unsigned long long *total;
    unsigned long long hit_cap;
    float thresh;
    int n, G, dim, n_qt, n_gt, self;
    int sw_q, sw_g, n_sq;                                 // super-tile edges in tiles, query super-tiles
    unsigned long long blocks;                            // places of all super-tiles; a workgroup takes every gridDim.x-th one
    unsigned q_bytes, g_bytes;
};

// one tile pair: linear id b -> (query tile, gallery tile), the GEMM, the threshold-and-compact epilogue
__device__ __forceinline__ void tile_pair(const RJArgs &a, unsigned long long b, char *smem, int tid, int lane, int wm, int wn) {
    // b = (super-tile, place inside it); super-tiles are sw_q x sw_g tile pairs and are walked in order, the places of one run together
    const unsigned per = (unsigned)(a.sw_q * a.sw_g);
    const unsigned long long sid = b / per;
    const int loc = (int)(b - sid * per);
    long long sq, sg;
    if (a.self) {
        // upper triangle of super-tiles, column by column: sid = sg (sg + 1) / 2 + sq with sq <= sg
        sg = (long long)((sqrt(8.0 * (double)sid + 1.0) - 1.0) * 0.5);
        while ((unsigned long long)sg * (sg + 1) / 2 > sid) sg--;
        while ((unsigned long long)(sg + 1) * (sg + 2) / 2 <= sid) sg++;
        sq = (long long)(sid - (unsigned long long)sg * (sg + 1) / 2);
    } else {
        sq = (long long)(sid % (unsigned)a.n_sq);           // the query super-tiles of one gallery super-tile run together
        sg = (long long)(sid / (unsigned)a.n_sq);
    }
    const int qt = (int)sq * a.sw_q + loc % a.sw_q, gt = (int)sg * a.sw_g + loc / a.sw_q;
    // (the ragged last super-tiles, and the lower half of a diagonal one: no such tile pair, nothing to do -- block-uniform, before any barrier)
    if (qt >= a.n_qt || gt >= a.n_gt || (a.self && gt < qt)) return;

    const auto rs_q = __builtin_amdgcn_make_buffer_rsrc((void *)a.q, 0, a.q_bytes, 0x00020000);
    const auto rs_g = __builtin_amdgcn_make_buffer_rsrc((void *)a.g, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    // per K-step a thread stages two 16-byte pieces of each operand: rows lrow and lrow + 64, group lgrp
    const int lrow = tid >> 2, lgrp = tid & 3;
    unsigned q_off[2], g_off[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int qr = qt * RT + lrow + 64 * i, gr = gt * RT + lrow + 64 * i;
        q_off[i] = qr < a.n ? (unsigned)qr * rowb + (unsigned)lgrp * 16u : ROOB;
        g_off[i] = gr < a.G ? (unsigned)gr * rowb + (unsigned)lgrp * 16u : ROOB;
    }
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);      // (row + 64: the same swizzle)

    u32x4 rq[2], rg[2];
    auto issue_loads = [&](int ks) {
        const unsigned kb = (unsigned)ks * (RCK * 2);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            rq[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_q, q_off[i] != ROOB ? q_off[i] + kb : ROOB, 0, 0);
            rg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_g, g_off[i] != ROOB ? g_off[i] + kb : ROOB, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
        char *dst = smem + buf * 2 * ROP_BYTES + st_off;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(u32x4 *)(dst + i * 64 * 64) = rq[i];
            *(u32x4 *)(dst + ROP_BYTES + i * 64 * 64) = rg[i];
        }
    };

    f32x4 acc[RMI][RNI];
#pragma unroll
    for (int mi = 0; mi < RMI; mi++)
#pragma unroll
        for (int ni = 0; ni < RNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ksteps = a.dim / RCK;
    issue_loads(0);
    store_tiles(0);
    __syncthreads();

    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = ROP_BYTES + (wn * 64 + frow) * 64 + grp;
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;
        if (more) issue_loads(ks + 1);
        const char *st = smem + cur * 2 * ROP_BYTES;
        half8 qf[RMI], gf[RNI];
#pragma unroll
        for (int mi = 0; mi < RMI; mi++) qf[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
        for (int ni = 0; ni < RNI; ni++) gf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
        for (int mi = 0; mi < RMI; mi++)
#pragma unroll
            for (int ni = 0; ni < RNI; ni++)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[mi], gf[ni], acc[mi][ni], 0, 0, 0);
        if (more) store_tiles(cur ^ 1);                     // last read in step ks - 1, behind that step's barrier
        __syncthreads();
    }

    // ---- threshold and compact: acc[mi][ni][j] = query (.. + 16 mi + 4 (lane >> 4) + j) x gallery row (.. + 16 ni + (lane & 15)) ----
    const int q0 = qt * RT + wm * 64 + (lane >> 4) * 4, g0 = gt * RT + wn * 64 + (lane & 15);
    auto is_hit = [&](float s, int q, int g) { return s >= a.thresh && s > 0.f && q < a.n && g < a.G && (!a.self || g > q); };
    unsigned long long mask = 0;                            // this lane's hits, bit 16 mi + 4 ni + j (kept as bits: 64 predicates would not fit the SGPRs)
#pragma unroll
    for (int mi = 0; mi < RMI; mi++)
#pragma unroll
        for (int ni = 0; ni < RNI; ni++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                mask |= (unsigned long long)is_hit(acc[mi][ni][j], q0 + mi * 16 + j, g0 + ni * 16) << (mi * 16 + ni * 4 + j);
    const int cnt = __popcll(mask);
    int inc = cnt;                                          // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    const int wave_hits = __shfl(inc, 63);
    if (wave_hits == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(a.total, (unsigned long long)wave_hits);
    base = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(base >> 32), 0) << 32) | (unsigned)__shfl((int)(unsigned)base, 0);
    unsigned long long slot = base + (unsigned)(inc - cnt);
#pragma unroll
    for (int mi = 0; mi < RMI; mi++)
#pragma unroll
        for (int ni = 0; ni < RNI; ni++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if ((mask >> (mi * 16 + ni * 4 + j)) & 1) {
                    if (slot < a.hit_cap) {
                        *(int2 *)(a.pairs + 2 * slot) = make_int2(q0 + mi * 16 + j, g0 + ni * 16);
                        a.scores[slot] = acc[mi][ni][j];
                    }
                    slot++;
                }
            }
}

// a workgroup takes every gridDim.x-th place (one each unless they outnumber what a launch may hold); the last K-step's barrier
// is also the one that frees the LDS buffers for the next pair
__global__ void __launch_bounds__(256) range_join128(const RJArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * ROP_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (unsigned long long b = blockIdx.x; b < a.blocks; b += gridDim.x) tile_pair(a, b, smem, tid, lane, wave & 1, wave >> 1);
}

}  // namespace
}  // namespace fid

extern "C" int fid_gallery_range(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, float thresh, int32_t *pairs_dev,
                                 float *scores_dev, long long hit_cap, uint64_t *total_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && pairs_dev && scores_dev && total_dev, "range: NULL context, gallery or output pointer");
    FID_REQUIRE(hit_cap > 0, "range: hit_cap %lld must be positive", hit_cap);
    FID_REQUIRE(!query_f16_dev || n > 0, "range: %d queries", n);
    FID_REQUIRE(!std::isnan(thresh), "range: the threshold is NaN");
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    RJArgs a{};
    a.self = query_f16_dev ? 0 : 1;
    a.q = a.self ? rows : query_f16_dev;
    a.g = rows;
    a.n = a.self ? G : n;
    a.G = G; a.dim = dim; a.thresh = thresh;
    a.pairs = pairs_dev; a.scores = scores_dev;
    a.total = (unsigned long long *)total_dev;
    a.hit_cap = (unsigned long long)hit_cap;
    const size_t q_rows = a.self ? (size_t)Gp : (size_t)a.n;
    FID_REQUIRE(dim > 0 && dim % RCK == 0, "range: embedding dim %d must be a multiple of %d", dim, RCK);
    FID_REQUIRE(q_rows * dim * 2 + (size_t)RT * dim * 2 < 0xFFFFFF00ull && (size_t)Gp * dim * 2 + (size_t)RT * dim * 2 < 0xFFFFFF00ull,
                "range: operand larger than 4 GiB");
    a.q_bytes = (unsigned)(q_rows * dim * 2);
    a.g_bytes = (unsigned)((size_t)Gp * dim * 2);
    a.n_qt = cdiv(a.n, RT);
    a.n_gt = cdiv(G, RT);
    // tile pairs are walked super-tile by super-tile (16 x 16 pairs share 32 operand tiles in the caches; one pair at a time streams a fresh
    // query tile from HBM per pair -- docs/FINDINGS.md, "range join").  FID_RANGE_SUPER=1 is the plain order (read per call: measurements)
    int sw = 16;
    if (const char *e = getenv("FID_RANGE_SUPER")) sw = std::max(1, std::min(64, atoi(e)));
    a.sw_q = std::min(sw, a.n_qt);
    a.sw_g = std::min(sw, a.n_gt);
    a.n_sq = cdiv(a.n_qt, a.sw_q);
    const long long n_sg = cdiv(a.n_gt, a.sw_g);
    a.blocks = (unsigned long long)(a.self ? n_sg * (n_sg + 1) / 2 : (long long)a.n_sq * n_sg) * (unsigned)(a.sw_q * a.sw_g);
    const unsigned grid = (unsigned)std::min<unsigned long long>(a.blocks, 1ull << 20);     // (grid x 256 threads stays below 2^32)
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_HIP(hipMemsetAsync(total_dev, 0, sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(range_join128, dim3(grid), dim3(256), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}
