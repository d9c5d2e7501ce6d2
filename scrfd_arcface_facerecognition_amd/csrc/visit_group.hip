// Grouping a batch of visits into persons, in visit order: the reference's process_visit_data loop as one asynchronous call.
//
// reference smart_face_recognition.py:1769-1951 runs, per visit, is_duplicate_image (:2618-2652, a k = 1 search at
// duplicate_similarity_threshold), search_person (:1619-1643, k = 5 at similarity_threshold), groups with the best hit when it reaches
// grouping_threshold_* (:1859-1861) and otherwise add_person (:1531-1602), which stores the embedding (qdrant_manager.py:91-136) -- so every
// new person is a candidate for every LATER visit and a visit that is merely recognised is not.  All three searches ask for the same thing,
// the best stored row; the loop is sequential only in WHICH rows are stored.  Three parts:
//
//   A  every visit against the store as it was at the call: the arg-max scan of fid_match (gemm_vs_gallery, CF_ARGMAX) into one packed
//      key per visit, sortable(score) << 32 | ~row -- the maximum key is the best score at the lowest row.  The only part that grows with G.
//   B  visits are cut into blocks of 128.  group_cross (block b, grid = b): the 128 x 128 tile of block b against block c < b of the QUERY
//      MATRIX ITSELF (the tile code of range_join.hip: mfma_f32_16x16x32_f16, register-staged buffer loads into a plain LDS double buffer,
//      one __syncthreads() per K-step, no hand-counted waits).  Epilogue: per query the maximum key over the columns whose visit was decided
//      NEW -- the key carries stored_row[j], the gallery row that visit was written to, so keys of A and B compare under one rule -- merged
//      by a 16-lane reduction and one 64-bit atomicMax per query and wave into the key array of A.  A block without a new person is skipped.
//   C  group_resolve (block b, ONE workgroup): the block's own 128 x 128 cosines by the same tile code into LDS (fp32, row stride 144
//      floats: the four query rows a fragment store covers fall into different banks), then wave 0 walks the visits in order.  Lane l owns
//      the candidates l and l + 64 (their stored rows live in its registers); per visit a wave max over the in-block candidates j < i, the
//      key of A / B, the rules of include/faceid.h, one lane writes the verdict.  No barrier inside the walk: one wave, state in registers.
//      Then all four waves copy the block's NEW rows into the gallery with plain 16-byte vector stores.
//
// Launch chain on the context's stream: prepare, A, C(0), B(1), C(1), B(2), C(2) ...  Order between blocks comes ONLY from stream order: no
// workgroup waits for another one, no flag is polled, nothing is launched cooperatively.
// Choices: B and C stay separate kernels (B is as wide as the batch is long, C is one workgroup; fused, b - 1 workgroups would idle through
// the walk), and part A runs ONCE (later blocks see earlier blocks' new persons through B, not through n / 128 gallery scans).
#include <cmath>

#include "conv.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int VT = 128, VCK = 32;                         // block of visits = tile edge, K-step
constexpr int VMI = 4, VNI = 4;                           // fragments of a wave: 64 x 64
constexpr int VOP_BYTES = VT * VCK * 2;                   // 8 KB per operand and step
constexpr unsigned VOOB = 0xFFFFFF00u;                    // past the query matrix (checked to be smaller)
constexpr int VS_LD = 144;                                // floats per row of the block's cosine matrix in LDS
constexpr int OFF_S = 2 * 2 * VOP_BYTES;                  // [128][144] fp32
constexpr int OFF_KEY = OFF_S + VT * VS_LD * 4;           // [128] keys of parts A / B
constexpr int OFF_NZ = OFF_KEY + VT * 8;                  // [128] "the query row has a non-zero element"
constexpr int OFF_ROW = OFF_NZ + VT * 4;                  // [128] gallery row of a NEW visit, else -1 (for the copy)
constexpr int RESOLVE_LDS = OFF_ROW + VT * 4;             // 108 544 bytes

struct VGArgs {
    const void *q;                                        // [n][dim] unit fp16
    void *gal;                                            // [Gp][dim]
    unsigned long long *keys;                             // [n]
    int32_t *stored_row, *nz, *state, *blk_new;           // [n], [n], {NEW so far, first DEFERRED visit}, [blocks] NEW visits per block
    const int32_t *new_rows;
    int32_t *verdict, *row, *summary;
    float *score;
    float dup, group, search;
    int n, G, dim, n_new_rows;
    unsigned q_bytes;
};

// (a NaN score gives key 0 = no candidate, as conv.hip's CF_ARGMAX epilogue does: a query row that is not a unit row must not win every later visit)
__device__ __forceinline__ unsigned long long make_key(float s, int row) {
    const unsigned u = __float_as_uint(s);
    const unsigned long long k = ((unsigned long long)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | (unsigned)~(unsigned)row;
    return s == s ? k : 0ull;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long k, int m) {
    return ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), m) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, m);
}

// visits row_a .. + 127 x visits row_b .. + 127 of the query matrix (rows >= n read as zeros):
// acc[mi][ni][j] = visit (row_a + 64 wm + 16 mi + 4 (lane >> 4) + j) x visit (row_b + 64 wn + 16 ni + (lane & 15)).  Ends behind a barrier.
__device__ __forceinline__ void tile_gemm(const VGArgs &a, int row_a, int row_b, char *smem, int tid, int lane, int wm, int wn,
                                          f32x4 (&acc)[VMI][VNI]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.q, 0, a.q_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    const int lrow = tid >> 2, lgrp = tid & 3;
    unsigned a_src[2], b_src[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ra = row_a + lrow + 64 * i, rb = row_b + lrow + 64 * i;
        a_src[i] = ra < a.n ? (unsigned)ra * rowb + (unsigned)lgrp * 16u : VOOB;
        b_src[i] = rb < a.n ? (unsigned)rb * rowb + (unsigned)lgrp * 16u : VOOB;
    }
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);
    u32x4 ra[2], rb[2];
    auto issue_loads = [&](int ks) {
        const unsigned kb = (unsigned)ks * (VCK * 2);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, a_src[i] != VOOB ? a_src[i] + kb : VOOB, 0, 0);
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_src[i] != VOOB ? b_src[i] + kb : VOOB, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
        char *dst = smem + buf * 2 * VOP_BYTES + st_off;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(u32x4 *)(dst + i * 64 * 64) = ra[i];
            *(u32x4 *)(dst + VOP_BYTES + i * 64 * 64) = rb[i];
        }
    };
#pragma unroll
    for (int mi = 0; mi < VMI; mi++)
#pragma unroll
        for (int ni = 0; ni < VNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = a.dim / VCK;
    issue_loads(0);
    store_tiles(0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = VOP_BYTES + (wn * 64 + frow) * 64 + grp;
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;
        if (more) issue_loads(ks + 1);
        const char *st = smem + cur * 2 * VOP_BYTES;
        half8 af[VMI], bf[VNI];
#pragma unroll
        for (int mi = 0; mi < VMI; mi++) af[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
        for (int ni = 0; ni < VNI; ni++) bf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
        for (int mi = 0; mi < VMI; mi++)
#pragma unroll
            for (int ni = 0; ni < VNI; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        if (more) store_tiles(cur ^ 1);                     // last read in step ks - 1, behind that step's barrier
        __syncthreads();
    }
}

// one wave per visit: does the row hold a non-zero element (the sign bit does not count: the -0.0 marker row of an empty slot is a zero row)?
// Also resets the per-call state.
__global__ void __launch_bounds__(256) group_prepare(const VGArgs a, int n_blocks) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid < n_blocks) a.blk_new[gid] = 0;
    if (gid == 0) { a.state[0] = 0; a.state[1] = a.n; }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.n) return;
    const unsigned *r = (const unsigned *)((const char *)a.q + (size_t)row * a.dim * 2);
    unsigned any = 0;
    for (int i = lane; i < a.dim / 2; i += 64) any |= r[i] & 0x7FFF7FFFu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= (unsigned)__shfl_xor((int)any, o);
    if (lane == 0) { a.nz[row] = any != 0u; a.stored_row[row] = -1; }
}

// part B: block b (queries) x block c = blockIdx.x < b (candidates)
__global__ void __launch_bounds__(256) group_cross(const VGArgs a, int b) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * VOP_BYTES];
    const int c = blockIdx.x;
    if (a.blk_new[c] == 0) return;                          // (block-uniform, before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    f32x4 acc[VMI][VNI];
    tile_gemm(a, b * VT, c * VT, smem, tid, lane, wm, wn, acc);
    const int q0 = b * VT + wm * 64 + (lane >> 4) * 4, c0 = c * VT + wn * 64 + (lane & 15);
    int sr[VNI];
#pragma unroll
    for (int ni = 0; ni < VNI; ni++) sr[ni] = a.stored_row[c0 + ni * 16];      // (c < b: every column is a visit of the batch)
#pragma unroll
    for (int mi = 0; mi < VMI; mi++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned long long key = 0ull;
#pragma unroll
            for (int ni = 0; ni < VNI; ni++) {
                const unsigned long long k = sr[ni] >= 0 ? make_key(acc[mi][ni][j], sr[ni]) : 0ull;
                key = k > key ? k : key;
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const unsigned long long k = shfl_xor_u64(key, o);
                key = k > key ? k : key;
            }
            const int qi = q0 + mi * 16 + j;
            if ((lane & 15) == 0 && qi < a.n && key != 0ull) atomicMax(a.keys + qi, key);
        }
}

// part C: block b, one workgroup
__global__ void __launch_bounds__(256) group_resolve(const VGArgs a, int b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int base = b * VT, m = min(VT, a.n - base);
    float *S = (float *)(smem + OFF_S);
    unsigned long long *keyl = (unsigned long long *)(smem + OFF_KEY);
    int *nzl = (int *)(smem + OFF_NZ), *rowl = (int *)(smem + OFF_ROW);
    if (tid < VT) {
        keyl[tid] = tid < m ? a.keys[base + tid] : 0ull;
        nzl[tid] = tid < m ? a.nz[base + tid] : 0;
        rowl[tid] = -1;
    }
    {
        f32x4 acc[VMI][VNI];
        tile_gemm(a, base, base, smem, tid, lane, wm, wn, acc);
        const int r0 = wm * 64 + (lane >> 4) * 4, c0 = wn * 64 + (lane & 15);
#pragma unroll
        for (int mi = 0; mi < VMI; mi++)
#pragma unroll
            for (int ni = 0; ni < VNI; ni++)
#pragma unroll
                for (int j = 0; j < 4; j++) S[(r0 + mi * 16 + j) * VS_LD + c0 + ni * 16] = acc[mi][ni][j];
    }
    __syncthreads();
    if (wave == 0) {
        // every lane holds the same cnt / first_def / in_block; lane l alone holds the stored rows of candidates l and l + 64
        int cnt = a.state[0], first_def = a.state[1], in_block = 0;
        int sr0 = -1, sr1 = -1;
        for (int i = 0; i < m; i++) {
            unsigned long long key = keyl[i];
            if (in_block > 0) {                             // (wave-uniform)
                const float s0 = S[i * VS_LD + lane], s1 = S[i * VS_LD + 64 + lane];
                const unsigned long long k0 = (lane < i && sr0 >= 0) ? make_key(s0, sr0) : 0ull;
                const unsigned long long k1 = (lane + 64 < i && sr1 >= 0) ? make_key(s1, sr1) : 0ull;
                unsigned long long k = k0 > k1 ? k0 : k1;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long t = shfl_xor_u64(k, o);
                    k = t > k ? t : k;
                }
                key = k > key ? k : key;
            }
            unsigned u = (unsigned)(key >> 32);
            u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
            float s = __uint_as_float(u);
            int r = (int)(~(unsigned)key);
            const bool hit = key != 0ull && s > 0.f && r >= 0 && r < a.G;       // "a score that is not > 0 is no hit": the rule of fid_match
            if (!hit) { s = 0.f; r = -1; }
            int v, out_row = -1;
            float out_score = 0.f;
            if (!nzl[i]) v = FID_VISIT_NO_FACE;
            else if (first_def < a.n) v = FID_VISIT_DEFERRED;
            else if (hit && s >= a.dup) { v = FID_VISIT_DUPLICATE; out_row = r; out_score = s; }
            else if (hit && s >= a.search && s >= a.group) { v = FID_VISIT_RECOGNISED; out_row = r; out_score = s; }
            else if (cnt >= a.n_new_rows) { v = FID_VISIT_DEFERRED; first_def = base + i; }
            else {
                v = FID_VISIT_NEW;
                const int nr = a.new_rows[cnt];
                cnt++;
                out_score = (hit && s >= a.search) ? s : 0.f;
                if (nr >= 0 && nr < a.G) {                  // a row outside the gallery is not stored and is nobody's candidate
                    out_row = nr;
                    in_block++;
                    if (lane == (i & 63)) { if (i < 64) sr0 = nr; else sr1 = nr; }
                }
            }
            if (lane == 0) { a.verdict[base + i] = v; a.row[base + i] = out_row; a.score[base + i] = out_score; }
        }
        if (lane < m) { a.stored_row[base + lane] = sr0; rowl[lane] = sr0; }
        if (lane + 64 < m) { a.stored_row[base + lane + 64] = sr1; rowl[lane + 64] = sr1; }
        if (lane == 0) {
            a.state[0] = cnt; a.state[1] = first_def; a.blk_new[b] = in_block;
            if (base + m >= a.n) { a.summary[0] = cnt; a.summary[1] = first_def; }
        }
    }
    __syncthreads();
    // the block's new persons enter the gallery: the query's fp16 row, bit for bit
    const int chunks = a.dim / 8;                           // 16-byte pieces per row
    for (int i = 0; i < m; i++) {
        const int r = rowl[i];
        if (r < 0) continue;
        const uint4 *src = (const uint4 *)((const char *)a.q + (size_t)(base + i) * a.dim * 2);
        uint4 *dst = (uint4 *)((char *)a.gal + (size_t)r * a.dim * 2);
        for (int k = tid; k < chunks; k += 256) dst[k] = src[k];
    }
}

}  // namespace
}  // namespace fid

extern "C" int fid_gallery_group(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, float dup_thresh, float group_thresh,
                                 float search_thresh, const int32_t *new_rows_dev, int n_new_rows, int32_t *verdict_dev, int32_t *row_dev,
                                 float *score_dev, int32_t *summary_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && new_rows_dev && verdict_dev && row_dev && score_dev && summary_dev,
                "group: NULL context, gallery, query, new_rows or output pointer");
    FID_REQUIRE(n > 0 && n <= FID_GROUP_MAX_VISITS, "group: %d visits (1 .. %d per call)", n, FID_GROUP_MAX_VISITS);
    FID_REQUIRE(n_new_rows >= 0, "group: n_new_rows %d is negative", n_new_rows);
    FID_REQUIRE(!std::isnan(dup_thresh) && !std::isnan(group_thresh) && !std::isnan(search_thresh), "group: a threshold is NaN");
    FID_REQUIRE(dup_thresh > 0.f && group_thresh > 0.f && search_thresh > 0.f,
                "group: thresholds %g / %g / %g must be > 0 (a hit needs a score > 0)", dup_thresh, group_thresh, search_thresh);
    FID_REQUIRE(((uintptr_t)query_f16_dev & 15) == 0, "group: the query rows must be 16-byte aligned");
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    FID_REQUIRE(dim > 0 && dim % VCK == 0, "group: embedding dim %d must be a multiple of %d", dim, VCK);
    FID_REQUIRE((size_t)n * dim * 2 + (size_t)VT * dim * 2 < 0xFFFFFF00ull, "group: query matrix larger than 4 GiB");
    const int n_blocks = cdiv(n, VT);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // scratch slot 2 (fid_match's key array; calls are serialised by the context's mutex and ordered by its stream).  The layout is the one of
    // the largest call, FID_GROUP_MAX_VISITS (1.3 MB), so the slot never grows between calls of this entry point: get_scratch synchronises
    // the stream when it has to REPLACE an arena, which can happen here once, if fid_match left a smaller one, and in a later, larger fid_match
    constexpr size_t NMAX = FID_GROUP_MAX_VISITS;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_stored = up(NMAX * 8), o_nz = o_stored + up(NMAX * 4), o_state = o_nz + up(NMAX * 4),
                 o_blk = o_state + 256, total = o_blk + up((NMAX / VT) * 4);
    void *ws;
    FID_TRY(get_scratch(ctx, 2, total, &ws));
    VGArgs a{};
    a.q = query_f16_dev; a.gal = rows;
    a.keys = (unsigned long long *)ws;
    a.stored_row = (int32_t *)((char *)ws + o_stored);
    a.nz = (int32_t *)((char *)ws + o_nz);
    a.state = (int32_t *)((char *)ws + o_state);
    a.blk_new = (int32_t *)((char *)ws + o_blk);
    a.new_rows = new_rows_dev;
    a.verdict = verdict_dev; a.row = row_dev; a.score = score_dev; a.summary = summary_dev;
    a.dup = dup_thresh; a.group = group_thresh; a.search = search_thresh;
    a.n = n; a.G = G; a.dim = dim; a.n_new_rows = n_new_rows;
    a.q_bytes = (unsigned)((size_t)n * dim * 2);
    FID_TRY(ensure_dyn_lds(ctx, (const void *)group_resolve, RESOLVE_LDS));
    FID_HIP(hipMemsetAsync(a.keys, 0, (size_t)n * 8, ctx->stream));
    hipLaunchKernelGGL(group_prepare, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a, n_blocks);
    FID_TRY(gallery_argmax_keys(ctx, g, query_f16_dev, n, a.keys));
    for (int b = 0; b < n_blocks; b++) {
        if (b > 0) hipLaunchKernelGGL(group_cross, dim3(b), dim3(256), 0, ctx->stream, a, b);
        hipLaunchKernelGGL(group_resolve, dim3(1), dim3(256), RESOLVE_LDS, ctx->stream, a, b);
    }
    FID_HIP(hipGetLastError());
    return FID_OK;
}
