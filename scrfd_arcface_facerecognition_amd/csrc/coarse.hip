// Two-stage gallery search: an exact int8 coarse scan for a shortlist of R rows per query, then the fp16 scores of just those rows.
//
// What vector stores ship as "quantised search with rescoring" (Qdrant, the role engine.VectorGallery stands in for, among them), with a
// quantisation rule (quant_core.h) that leaves nothing to the platform: power-of-two row scales and integer sums, so the shortlist is predictable
// to the bit for every input -- tests/coarse_oracle.py restates it in numpy.
//
//   quantise = one wave per row: the largest magnitude by a wave maximum over fp16 bit patterns, the row's exponent from its bits, one rounding
//              per element; four codes leave a lane as one 32-bit vector store.
//   scan     = topk_scan's kernel with int8 operands: a 128-query x 128-row tile, four waves of 4 x 4 mfma_i32_16x16x64_i8 fragments, register-
//              staged buffer loads into the XOR-swizzled LDS double buffer.  A K-step of 64 int8 is the 64 bytes per row that 32 fp16 are, so the
//              staging addresses, the fragment reads (16 bytes per lane, group lane >> 4 of row lane & 15) and the 32 KB of LDS are topk_scan's
//              and there are half as many K-steps.  Both operands go through the same K map, so whichever K index the instruction gives byte j
//              of a lane's fragment, the product sums over matching pairs.  The i32 sums go through the pass buffer as they are; the selecting
//              thread scales them by 2^(e_q + e_g) (the tile's 128 row exponents sit in 128 more bytes of LDS) -- exact, see quant_core.h --
//              and keeps the sorted key list of topk_scan.  Only dot > 0 makes a key.
//   merge    = topk_merge as it is (topk_keys.h): it only sees keys.
//   rerank   = one wave per query: for each of its R keys the dot product of the two fp16 rows, fp32 fmaf in a fixed order (lane l takes elements
//              8 l .. 8 l + 7 and, beyond dim 512, 512 + 8 l ..; then a butterfly sum), the key rebuilt with that score, and the R keys written
//              in descending order by rank counting.  No atomics.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gallery.h"
#include "quant_core.h"
#include "topk_keys.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int TT = 128, TCK = 64;                         // tile edge (both operands), K-step in int8 elements
constexpr int TMI = 4, TNI = 4;                           // fragments of a wave: 64 queries x 64 gallery rows
constexpr int TOP_BYTES = TT * TCK;                       // 8 KB per operand and step
constexpr unsigned TOOB = 0xFFFFFF00u;                    // past every operand (both are checked to be smaller)
constexpr size_t CAND_BYTES_MAX = 256ull << 20;           // topk_scan's limit for the lists of one launch

inline bool coarse_dim_ok(int dim) { return dim > 0 && dim % TCK == 0 && dim <= FID_QUANT_DIM_MAX; }

// ---- quantise ----------------------------------------------------------------------------------------------------------------------------------
// rows != NULL: row i of the call is gallery row rows[i] (skipped outside [0, cap)); otherwise row i
__global__ void __launch_bounds__(256) quant_rows(const uint16_t *__restrict__ unit, const int *__restrict__ rows, int n, int dim, int cap,
                                                  int8_t *__restrict__ codes, int8_t *__restrict__ exps) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int r = rows ? rows[i] : i;
    if (r < 0 || r >= cap) return;
    const uint16_t *src = unit + (size_t)r * dim;
    unsigned mx = 0;
    for (int j = lane * 4; j < dim; j += 256) {
        const uint2 v = *(const uint2 *)(src + j);
        mx = max(max(mx, v.x & 0x7FFFu), max((v.x >> 16) & 0x7FFFu, max(v.y & 0x7FFFu, (v.y >> 16) & 0x7FFFu)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    bool live;
    const int e = fid_quant_row_exp(mx, &live);
    const float inv = fid_quant_pow2(-e);
    for (int j = lane * 4; j < dim; j += 256) {
        const uint2 v = *(const uint2 *)(src + j);
        const unsigned c0 = (uint8_t)fid_quant_code((uint16_t)(v.x & 0xFFFFu), inv, live), c1 = (uint8_t)fid_quant_code((uint16_t)(v.x >> 16), inv, live);
        const unsigned c2 = (uint8_t)fid_quant_code((uint16_t)(v.y & 0xFFFFu), inv, live), c3 = (uint8_t)fid_quant_code((uint16_t)(v.y >> 16), inv, live);
        *(unsigned *)(codes + (size_t)r * dim + j) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
    if (lane == 0) exps[r] = (int8_t)e;
}

void launch_quant(fid_ctx *ctx, const void *unit, const int *rows, int n, int dim, int cap, int8_t *codes, int8_t *exps) {
    hipLaunchKernelGGL(quant_rows, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, (const uint16_t *)unit, rows, n, dim, cap, codes, exps);
}

// ---- scan --------------------------------------------------------------------------------------------------------------------------------------
struct CSArgs {
    const void *q, *g;                                    // int8 codes [n][dim], [Gp][dim]
    const int8_t *qe, *ge;                                // their exponents
    u64 *cand;                                            // [n][S][2][KP]
    int n, G, dim, n_qt, n_gt, tps, S, col0;
    unsigned q_bytes, g_bytes;
};

template <int KP>
__global__ void __launch_bounds__(256) coarse_scan(const CSArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TOP_BYTES];
    __shared__ __attribute__((aligned(16))) int8_t tile_e[TT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int qt = (int)(blockIdx.x % (unsigned)a.n_qt), sl = (int)(blockIdx.x / (unsigned)a.n_qt);
    const int gt_end = min(sl * a.tps + a.tps, a.n_gt);

    const auto rs_q = __builtin_amdgcn_make_buffer_rsrc((void *)a.q, 0, a.q_bytes, 0x00020000);
    const auto rs_g = __builtin_amdgcn_make_buffer_rsrc((void *)a.g, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim;
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
    const int my_e = qt * TT + myq < a.n ? (int)a.qe[qt * TT + myq] : 0;
    u64 best[KP];
#pragma unroll
    for (int j = 0; j < KP; j++) best[j] = 0ull;
    float floor_s = 0.f;                                    // the score of best[KP - 1] (0 while the list is not full)
    int *sc = (int *)smem;                                  // the pass buffer: [64 rows][128 queries] i32 = the 32 KB of staging

    for (int gt = sl * a.tps; gt < gt_end; gt++) {
        unsigned g_off[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int gr = gt * TT + lrow + 64 * i;
            g_off[i] = gr < a.G ? (unsigned)gr * rowb + (unsigned)lgrp * 16u : TOOB;
        }
        // (the exponents of the tile before were last read in front of its last barrier; the first barrier below publishes these)
        if (tid < TT) tile_e[tid] = gt * TT + tid < a.G ? a.ge[gt * TT + tid] : (int8_t)0;
        u32x4 rq[2], rg[2];
        auto issue_loads = [&](int ks) {
            const unsigned kb = (unsigned)ks * TCK;
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

        i32x4 acc[TMI][TNI];
#pragma unroll
        for (int mi = 0; mi < TMI; mi++)
#pragma unroll
            for (int ni = 0; ni < TNI; ni++) acc[mi][ni] = i32x4{0, 0, 0, 0};

        issue_loads(0);
        store_tiles(0);                                     // (the pass buffer of the tile before was last read behind a barrier)
        __syncthreads();
        for (int ks = 0; ks < ksteps; ks++) {
            const int cur = ks & 1;
            const bool more = ks + 1 < ksteps;
            if (more) issue_loads(ks + 1);
            const char *st = smem + cur * 2 * TOP_BYTES;
            i32x4 qf[TMI], gf[TNI];
#pragma unroll
            for (int mi = 0; mi < TMI; mi++) qf[mi] = *(const i32x4 *)(st + a_off + mi * 1024);
#pragma unroll
            for (int ni = 0; ni < TNI; ni++) gf[ni] = *(const i32x4 *)(st + b_off + ni * 1024);
#pragma unroll
            for (int mi = 0; mi < TMI; mi++)
#pragma unroll
                for (int ni = 0; ni < TNI; ni++)
                    acc[mi][ni] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf[mi], gf[ni], acc[mi][ni], 0, 0, 0);
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
                        *(i32x4 *)(sc + r * TT + ((qg ^ (r & 31)) << 2)) = acc[mi][ni];
                    }
            }
            __syncthreads();
            const int row0 = a.col0 + gt * TT + pass * 64;
#pragma unroll 1
            for (int r = half * 32; r < half * 32 + 32; r += 4) {
                int d[4];
#pragma unroll
                for (int e = 0; e < 4; e++) d[e] = sc[(r + e) * TT + (((myq >> 2) ^ ((r + e) & 31)) << 2) + (myq & 3)];
                if (max(max(d[0], d[1]), max(d[2], d[3])) > 0) {
                    const unsigned ew = *(const unsigned *)(tile_e + pass * 64 + r);       // the four rows' exponents
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float s = (float)d[e] * fid_quant_pow2(my_e + (int)(int8_t)(ew >> (8 * e)));
                        if (d[e] > 0 && s >= floor_s) {
                            const u64 key = make_key(s, row0 + r + e);
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

// ---- rerank ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rerank_rows(const _Float16 *__restrict__ q, const _Float16 *__restrict__ gal, int n, int G, int dim, int R,
                                                   int first_row, const u64 *__restrict__ kin, u64 *__restrict__ kout) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= n) return;
    const bool has0 = lane * 8 < dim, has1 = 512 + lane * 8 < dim;        // dim <= 1024: at most two pieces per lane
    half8 qv0 = {0, 0, 0, 0, 0, 0, 0, 0}, qv1 = {0, 0, 0, 0, 0, 0, 0, 0};
    if (has0) qv0 = *(const half8 *)(q + (size_t)qi * dim + lane * 8);
    if (has1) qv1 = *(const half8 *)(q + (size_t)qi * dim + 512 + lane * 8);
    u64 mine = 0ull;
    for (int t = 0; t < R; t++) {
        const u64 key = kin[(size_t)qi * R + t];
        const int row = (int)(~(unsigned)key) - first_row;
        u64 nk = 0ull;
        if (key != 0ull && row >= 0 && row < G) {           // (the same for the whole wave)
            const _Float16 *gr = gal + (size_t)row * dim;
            float acc = 0.f;
            if (has0) {
                const half8 gv = *(const half8 *)(gr + lane * 8);
#pragma unroll
                for (int i = 0; i < 8; i++) acc = fmaf((float)qv0[i], (float)gv[i], acc);
            }
            if (has1) {
                const half8 gv = *(const half8 *)(gr + 512 + lane * 8);
#pragma unroll
                for (int i = 0; i < 8; i++) acc = fmaf((float)qv1[i], (float)gv[i], acc);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (acc > 0.f) nk = make_key(acc, first_row + row);            // (a NaN fails the comparison)
        }
        if (lane == t) mine = nk;
    }
    // the rank of this lane's key among the R: keys of different rows differ; zeros (and a caller's repeated key) keep their order
    int rank = 0;
    for (int t = 0; t < R; t++) {
        const u64 other = ((u64)(unsigned)__shfl((int)(unsigned)(mine >> 32), t) << 32) | (unsigned)__shfl((int)(unsigned)mine, t);
        rank += (other > mine || (other == mine && t < lane)) ? 1 : 0;
    }
    if (lane < R) kout[(size_t)qi * R + rank] = mine;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// quantise the queries into the scratch arena, scan, and merge the lists into keys [n, R] (the context's mutex is held, the gallery has its
// quantised copy).  keys_out == NULL: the arena's front holds `arena_arrays` key arrays [n, R]; the keys go to the first and *arena names it.
int coarse_scan_keys(fid_ctx *ctx, fid_gallery *g, const void *q, int n, int R, int first_row, u64 *keys_out, int arena_arrays, u64 **arena) {
    const int G = g->G, Gp = g->Gp, dim = g->dim;
    const int KP = list_len(R);
    const int n_gt = cdiv(G, TT);
    // the slices of topk_scan (scan_keys): about two workgroups per CU, never more than gallery tiles; FID_TOPK_SLICES (read per call) forces S
    long long S = std::max(1, 2 * ctx->num_cus / cdiv(n, TT));
    if (const char *e = getenv("FID_TOPK_SLICES")) S = std::max(1, atoi(e));
    const size_t list_bytes = (size_t)2 * KP * 8;           // per query and slice
    S = std::min<long long>({S, (long long)n_gt, (long long)(CAND_BYTES_MAX / (TT * list_bytes))});
    const int tps = cdiv(n_gt, (int)S);
    S = cdiv(n_gt, tps);                                    // no empty slice
    long long chunk = std::min<long long>(n, (long long)(CAND_BYTES_MAX / (S * list_bytes)) / TT * TT);
    chunk = std::min<long long>(chunk, (long long)(0xFFFFFF00ull / (size_t)dim) / TT * TT - TT);
    FID_REQUIRE(chunk > 0 && (size_t)Gp * dim + (size_t)TT * dim < 0xFFFFFF00ull, "coarse: operand larger than 4 GiB");
    const size_t keys_bytes = keys_out ? 0 : (size_t)arena_arrays * up256((size_t)n * R * 8);
    const size_t code_bytes = up256((size_t)n * dim), exp_bytes = up256((size_t)n);
    void *ws;
    FID_TRY(get_scratch(ctx, 3, keys_bytes + code_bytes + exp_bytes + (size_t)chunk * S * list_bytes, &ws));
    if (!keys_out) keys_out = *arena = (u64 *)ws;
    int8_t *qc = (int8_t *)ws + keys_bytes, *qe = qc + code_bytes;
    launch_quant(ctx, q, nullptr, n, dim, n, qc, qe);
    CSArgs a{};
    a.g = g->codes_i8; a.ge = g->exps_i8; a.G = G; a.dim = dim; a.col0 = first_row;
    a.cand = (u64 *)(qe + exp_bytes);
    a.n_gt = n_gt; a.tps = tps; a.S = (int)S;
    a.g_bytes = (unsigned)((size_t)Gp * dim);
    for (long long q0 = 0; q0 < n; q0 += chunk) {
        const int m = (int)std::min<long long>(chunk, n - q0);
        a.q = qc + (size_t)q0 * dim;
        a.qe = qe + q0;
        a.n = m;
        a.n_qt = cdiv(m, TT);
        a.q_bytes = (unsigned)((size_t)m * dim);
        const dim3 grid((unsigned)(a.n_qt * a.S));
        switch (KP) {
            case 8: hipLaunchKernelGGL(coarse_scan<8>, grid, dim3(256), 0, ctx->stream, a); break;
            case 16: hipLaunchKernelGGL(coarse_scan<16>, grid, dim3(256), 0, ctx->stream, a); break;
            default: hipLaunchKernelGGL(coarse_scan<32>, grid, dim3(256), 0, ctx->stream, a); break;
        }
        const int count = (int)(S * 2 * KP);
        launch_merge(ctx, a.cand, 1, 0, count, count, m, R, 0x7FFFFFFF, 0.f, keys_out + (size_t)q0 * R, nullptr, nullptr);
    }
    FID_HIP(hipGetLastError());
    return FID_OK;
}

void launch_rerank(fid_ctx *ctx, fid_gallery *g, const void *q, int n, int R, int first_row, const u64 *kin, u64 *kout) {
    hipLaunchKernelGGL(rerank_rows, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, (const _Float16 *)q, (const _Float16 *)g->unit_f16, n, g->G, g->dim,
                       R, first_row, kin, kout);
}

int require_quantised(fid_gallery *g, const char *who) {
    if (!g->codes_i8 || !g->exps_i8) {
        set_error("%s: the gallery has no quantised copy (fid_gallery_quantize)", who);
        return FID_E_STATE;
    }
    return FID_OK;
}

}  // namespace

void requantize_rows(fid_ctx *ctx, fid_gallery *g, const int *rows_dev, int n) {
    launch_quant(ctx, g->unit_f16, rows_dev, n, g->dim, g->G, g->codes_i8, g->exps_i8);
}

}  // namespace fid

extern "C" {

int fid_quantize_rows_i8_host(const uint16_t *unit_f16, int n, int dim, int8_t *codes, int8_t *exps) {
    FID_REQUIRE(unit_f16 && codes && exps, "quantise: NULL rows, codes or exponents pointer");
    FID_REQUIRE(n > 0 && fid::coarse_dim_ok(dim), "quantise: %d rows of dim %d (dim must be a multiple of 64, at most %d)", n, dim, FID_QUANT_DIM_MAX);
    fid_quantize_rows_i8_table_host(unit_f16, n, dim, codes, exps);
    return FID_OK;
}

int fid_quantize_rows_i8(fid_ctx *ctx, const void *unit_f16_dev, int n, int dim, int8_t *codes_dev, int8_t *exps_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && unit_f16_dev && codes_dev && exps_dev, "quantise: NULL context, rows, codes or exponents pointer");
    FID_REQUIRE(n > 0 && coarse_dim_ok(dim), "quantise: %d rows of dim %d (dim must be a multiple of 64, at most %d)", n, dim, FID_QUANT_DIM_MAX);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    launch_quant(ctx, unit_f16_dev, nullptr, n, dim, n, codes_dev, exps_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_gallery_quantize(fid_ctx *ctx, fid_gallery *g) {
    using namespace fid;
    FID_REQUIRE(ctx && g, "gallery quantise: NULL context or gallery");
    FID_REQUIRE(coarse_dim_ok(g->dim), "gallery quantise: dim %d must be a multiple of 64, at most %d", g->dim, FID_QUANT_DIM_MAX);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    if (!g->codes_i8) FID_HIP(hipMalloc((void **)&g->codes_i8, (size_t)g->Gp * g->dim + 256));
    if (!g->exps_i8) FID_HIP(hipMalloc((void **)&g->exps_i8, (size_t)g->Gp + 256));
    launch_quant(ctx, g->unit_f16, nullptr, g->Gp, g->dim, g->Gp, g->codes_i8, g->exps_i8);    // (rows >= G are zero: code 0, exponent 0)
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_gallery_quant_data(fid_gallery *g, const int8_t **codes_dev, const int8_t **exps_dev) {
    FID_REQUIRE(g && codes_dev && exps_dev, "bad args");
    FID_TRY(fid::require_quantised(g, "quant data"));
    *codes_dev = g->codes_i8;
    *exps_dev = g->exps_i8;
    return FID_OK;
}

int fid_coarse_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int R, int first_row, uint64_t *keys_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && keys_dev, "coarse keys: NULL context, gallery, query or output pointer");
    FID_REQUIRE(n > 0, "coarse keys: %d queries", n);
    FID_REQUIRE(R >= 1 && R <= FID_TOPK_MAX, "coarse keys: R = %d is outside 1 .. %d", R, FID_TOPK_MAX);
    FID_REQUIRE(first_row >= 0 && (long long)first_row + g->Gp < 0x7FFFFFFFll, "coarse keys: global gallery index overflows 31 bits");
    FID_REQUIRE(coarse_dim_ok(g->dim), "coarse keys: dim %d must be a multiple of 64, at most %d", g->dim, FID_QUANT_DIM_MAX);
    FID_TRY(require_quantised(g, "coarse keys"));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    return coarse_scan_keys(ctx, g, query_f16_dev, n, R, first_row, (u64 *)keys_dev, 0, nullptr);
}

int fid_rerank_keys(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int R, int first_row, const uint64_t *keys_in_dev,
                    uint64_t *keys_out_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && keys_in_dev && keys_out_dev, "rerank: NULL context, gallery, query or key pointer");
    FID_REQUIRE(keys_in_dev != keys_out_dev, "rerank: the keys cannot be reranked in place");
    FID_REQUIRE(n > 0, "rerank: %d queries", n);
    FID_REQUIRE(R >= 1 && R <= FID_TOPK_MAX, "rerank: R = %d is outside 1 .. %d", R, FID_TOPK_MAX);
    FID_REQUIRE(first_row >= 0 && (long long)first_row + g->Gp < 0x7FFFFFFFll, "rerank: global gallery index overflows 31 bits");
    FID_REQUIRE(g->dim <= FID_QUANT_DIM_MAX, "rerank: dim %d is above %d", g->dim, FID_QUANT_DIM_MAX);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    launch_rerank(ctx, g, query_f16_dev, n, R, first_row, (const u64 *)keys_in_dev, (u64 *)keys_out_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// exactly fid_coarse_keys(first_row = 0), fid_rerank_keys and fid_topk_merge(parts = 1): one code path for the sharded and the unsharded search
int fid_gallery_search_coarse(fid_ctx *ctx, fid_gallery *g, const void *query_f16_dev, int n, int k, int R, float thresh, int32_t *idx_dev,
                              float *score_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && query_f16_dev && idx_dev && score_dev, "coarse search: NULL context, gallery, query or output pointer");
    FID_REQUIRE(n > 0, "coarse search: %d queries", n);
    FID_REQUIRE(k >= 1 && k <= R && R <= FID_TOPK_MAX, "coarse search: need 1 <= k <= R <= %d, got k = %d, R = %d", FID_TOPK_MAX, k, R);
    FID_REQUIRE(!std::isnan(thresh), "coarse search: the threshold is NaN");
    FID_REQUIRE((long long)g->Gp < 0x7FFFFFFFll, "coarse search: global gallery index overflows 31 bits");
    FID_REQUIRE(coarse_dim_ok(g->dim), "coarse search: dim %d must be a multiple of 64, at most %d", g->dim, FID_QUANT_DIM_MAX);
    FID_TRY(require_quantised(g, "coarse search"));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    u64 *keys = nullptr;
    FID_TRY(coarse_scan_keys(ctx, g, query_f16_dev, n, R, 0, nullptr, 2, &keys));
    u64 *exact = (u64 *)((char *)keys + up256((size_t)n * R * 8));
    launch_rerank(ctx, g, query_f16_dev, n, R, 0, keys, exact);
    launch_merge(ctx, exact, 1, (long long)n * R, R, R, n, k, g->G, thresh, nullptr, idx_dev, score_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // extern "C"
