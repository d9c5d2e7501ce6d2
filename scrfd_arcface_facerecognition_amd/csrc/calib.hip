// Genuine / impostor score distributions of labelled stored faces: "how are same-person and different-person cosines distributed, and which
// stored faces are probably mislabelled" as ONE asynchronous call (include/faceid.h has the rule in full; tests/calib_oracle.py is its
// executable form).  What a user calibrates the library's thresholds with.
//
//     takes part  = row inside the gallery, a non-zero element (the sign bit does not count), label >= 0
//     pair (i, j) = every unordered pair i < j of positions that take part, once; s = the fp32 cosine of the two stored fp16 rows
//     class       = GENUINE when the two labels are equal, IMPOSTOR otherwise; a non-finite s is counted in summary[3] and in no bin
//     bin         = fid_hist_bin (calib_core.h): one rounded fp32 multiply, exact for a power-of-two bin count
//     imp_via[k]  = the position of another label with the HIGHEST finite score, gen_via[k] = the position of the same label with the LOWEST;
//                   the lowest position among equal scores
//
// Launch chain on the context's stream: prepare, pass, finish.  Order comes ONLY from stream order: no workgroup waits for another one, no flag
// is polled, nothing is launched cooperatively (the discipline of dedup.hip / cluster.hip).
//
//   hist_prepare  one wave per position: does it take part?  Its effective label (the label, or -1) is parked in gen_via_dev until hist_finish
//                 overwrites it, so the pass reads ONE word per position; keys = 0 (impostor, raised by atomicMax) and ~0 (genuine, lowered by
//                 atomicMin); hist and summary are zeroed.
//   hist_pass     the upper triangle of 128 x 128 position tiles, diagonal tiles included, only pairs i < j, walked super-tile by super-tile
//                 (range_join.hip / cluster.hip).  The tile code is a copy of cluster.hip's tile_gemm (register-staged buffer loads, a plain LDS
//                 double buffer, one __syncthreads() per K-step, no hand-counted waits): the same sums as the clustering.  Epilogue per wave on
//                 its 64 x 64 accumulators: the labels of its 64 rows and 64 columns once, class and bin per element, counts into a
//                 per-workgroup LDS histogram of uint32 counters [2][bins], every lane one LDS atomicAdd per element (PEEL = 0, the default).
//                 PEEL = 4 (FID_HIST_PEEL=4) aggregates the lanes of a wave that hit the same counter first -- four rounds of "take the first
//                 live lane's counter, ballot who shares it, ONE add of the lane count", the rest lane by lane; measured, it is the slower
//                 of the two on concentrated and on spread scores alike (docs/FINDINGS.md "score distributions"), so it is kept for
//                 measurements only.  The LDS histogram is flushed to hist_dev with 64-bit integer atomicAdd, non-zero counters only, whenever the workgroup leaves a
//                 super-tile and at its end: at most 256 tiles x 16 384 pairs per flush, below 2^32.  Integer sums do not depend on the
//                 arrival order.  The hard-pair keys are reduced per row and per column inside the wave (dedup_cross), then ONE 64-bit
//                 atomicMax / atomicMin per position and wave.
//   hist_finish   one thread per position: keys -> via / score; positions that took part are counted; the first workgroup adds the class
//                 totals up from the histogram.
//
// No n x n matrix and no pair list exists anywhere; the gallery is never written.  Scratch: the two keys, 16 bytes per position.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "calib_core.h"
#include "common.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int HT = 128, HCK = 32;                         // tile edge in positions, K-step
constexpr int HMI = 4, HNI = 4;                           // fragments of a wave: 64 x 64
constexpr int HOP_BYTES = HT * HCK * 2;                   // 8 KB per operand and step
constexpr int HTILE_BYTES = 2 * 2 * HOP_BYTES;            // the double buffer of both operands; the LDS histogram lies behind it
constexpr unsigned HOOB = 0xFFFFFF00u;                    // past the gallery (checked to be smaller): such a load returns zeros
constexpr int HSUPER = 16;                                // super-tile edge in tiles (range_join.hip)

struct HArgs {
    void *gal;                                            // [Gp][dim] unit fp16, read only
    const int32_t *rows;                                  // [n] gallery row of every position, or NULL: position k is row k
    const int32_t *labels;                                // [n]
    u64 *ikey, *gkey;                                     // [n] each
    u64 *hist, *summary;                                  // [2][bins], [4]
    int32_t *imp_via, *eff;                               // eff = gen_via_dev: the effective label between prepare and finish
    float *imp_score, *gen_score;
    int bins, n, G, dim, n_t, sw;
    u64 blocks;                                           // places of all super-tiles; a workgroup takes every gridDim.x-th one
    unsigned g_bytes;
};

__device__ __forceinline__ int row_of(const HArgs &a, int pos) { return a.rows ? a.rows[pos] : pos; }

// cluster.hip's tile_gemm: positions pos_a .. + 127 x positions pos_b .. + 127 (a position >= n or with a row outside the gallery reads as zeros):
// acc[mi][ni][j] = position (pos_a + 64 wm + 16 mi + 4 (lane >> 4) + j) x position (pos_b + 64 wn + 16 ni + (lane & 15)).  Ends behind a barrier.
__device__ __forceinline__ void tile_gemm(const HArgs &a, int pos_a, int pos_b, char *smem, int tid, int lane, int wm, int wn,
                                          f32x4 (&acc)[HMI][HNI]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.gal, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    const int lrow = tid >> 2, lgrp = tid & 3;
    unsigned a_src[2], b_src[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pa = pos_a + lrow + 64 * i, pb = pos_b + lrow + 64 * i;
        const int ra = pa < a.n ? row_of(a, pa) : -1, rb = pb < a.n ? row_of(a, pb) : -1;
        a_src[i] = (ra >= 0 && ra < a.G) ? (unsigned)ra * rowb + (unsigned)lgrp * 16u : HOOB;
        b_src[i] = (rb >= 0 && rb < a.G) ? (unsigned)rb * rowb + (unsigned)lgrp * 16u : HOOB;
    }
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);
    u32x4 ra[2], rb[2];
    auto issue_loads = [&](int ks) {
        const unsigned kb = (unsigned)ks * (HCK * 2);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, a_src[i] != HOOB ? a_src[i] + kb : HOOB, 0, 0);
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_src[i] != HOOB ? b_src[i] + kb : HOOB, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
        char *dst = smem + buf * 2 * HOP_BYTES + st_off;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(u32x4 *)(dst + i * 64 * 64) = ra[i];
            *(u32x4 *)(dst + HOP_BYTES + i * 64 * 64) = rb[i];
        }
    };
#pragma unroll
    for (int mi = 0; mi < HMI; mi++)
#pragma unroll
        for (int ni = 0; ni < HNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = a.dim / HCK;
    issue_loads(0);
    store_tiles(0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = HOP_BYTES + (wn * 64 + frow) * 64 + grp;
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;
        if (more) issue_loads(ks + 1);
        const char *st = smem + cur * 2 * HOP_BYTES;
        half8 af[HMI], bf[HNI];
#pragma unroll
        for (int mi = 0; mi < HMI; mi++) af[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
        for (int ni = 0; ni < HNI; ni++) bf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
        for (int mi = 0; mi < HMI; mi++)
#pragma unroll
            for (int ni = 0; ni < HNI; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        if (more) store_tiles(cur ^ 1);                     // last read in step ks - 1, behind that step's barrier
        __syncthreads();
    }
}

// one wave per position: does it take part?  Also the per-call state of the position, and the zeroes of hist and summary.
__global__ void __launch_bounds__(256) hist_prepare(const HArgs a) {
    const unsigned words = 2u * (unsigned)a.bins + FID_HIST_SUMMARY_WORDS;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < words; i += gridDim.x * 256u) {
        if (i < 2u * (unsigned)a.bins) a.hist[i] = 0ull; else a.summary[i - 2u * (unsigned)a.bins] = 0ull;
    }
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pos >= a.n) return;
    const int row = row_of(a, pos);
    unsigned any = 0;
    if (row >= 0 && row < a.G) {                            // (wave-uniform)
        const unsigned *r = (const unsigned *)((const char *)a.gal + (size_t)row * a.dim * 2);
        for (int i = lane; i < a.dim / 2; i += 64) any |= r[i] & 0x7FFF7FFFu;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= (unsigned)__shfl_xor((int)any, o);
    if (lane == 0) {
        const int label = a.labels[pos];
        a.eff[pos] = (any != 0u && label >= 0) ? label : -1;
        a.ikey[pos] = 0ull;
        a.gkey[pos] = ~0ull;
    }
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 k, int o) {
    return ((u64)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), o) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, o);
}

// one count into counter idx of the workgroup's LDS histogram for every lane with idx >= 0 (the whole wave calls this together).  PEEL rounds of
// aggregation: the counter of the first live lane, a ballot of the lanes that share it, one add of their number by that lane.
template <int PEEL>
__device__ __forceinline__ void hist_add(unsigned *h, int idx, int lane) {
#pragma unroll
    for (int p = 0; p < PEEL; p++) {
        const u64 live = __ballot(idx >= 0);
        if (live != 0) {                                    // (wave-uniform)
            const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
            const int first = __builtin_amdgcn_readlane(idx, lead);
            const u64 same = __ballot(idx == first);
            if (lane == lead) atomicAdd(h + first, (unsigned)__popcll(same));
            if (idx == first) idx = -1;
        }
    }
    if (idx >= 0) atomicAdd(h + idx, 1u);
}

// the epilogue of one wave on its 64 x 64 part of tile pair (ti, tj)
template <int PEEL>
__device__ __forceinline__ void tile_epilogue(const HArgs &a, const f32x4 (&acc)[HMI][HNI], unsigned *h, int ti, int tj, int lane, int wm, int wn) {
    if (ti == tj && wm > wn) return;                        // below the diagonal: no pair with row < column (wave-uniform; no barrier follows)
    const int r0 = ti * HT + wm * 64 + (lane >> 4) * 4, c0 = tj * HT + wn * 64 + (lane & 15);
    int cl[HNI];
#pragma unroll
    for (int ni = 0; ni < HNI; ni++) {
        const int c = c0 + ni * 16;
        cl[ni] = c < a.n ? a.eff[c] : -1;
    }
    u64 cik[HNI] = {0ull, 0ull, 0ull, 0ull}, cgk[HNI] = {~0ull, ~0ull, ~0ull, ~0ull};
    unsigned non_finite = 0;
#pragma unroll
    for (int mi = 0; mi < HMI; mi++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = r0 + mi * 16 + j;
            const int rl = r < a.n ? a.eff[r] : -1;
            u64 rik = 0ull, rgk = ~0ull;
#pragma unroll
            for (int ni = 0; ni < HNI; ni++) {
                const int c = c0 + ni * 16;
                const unsigned u = __float_as_uint(acc[mi][ni][j]);
                const bool pair = r < c && rl >= 0 && cl[ni] >= 0;                     // (cl >= 0: c < n, and then r < n)
                const bool fin = fid_hist_finite(u);
                const bool imp = rl != cl[ni];
                non_finite += pair && !fin;
                int idx = -1;
                if (pair && fin) {
                    idx = (imp ? a.bins : 0) + fid_hist_bin(acc[mi][ni][j], a.bins);
                    if (imp) {
                        const u64 kr = fid_hist_imp_key(u, c), kc = fid_hist_imp_key(u, r);
                        rik = kr > rik ? kr : rik;
                        cik[ni] = kc > cik[ni] ? kc : cik[ni];
                    } else {
                        const u64 kr = fid_hist_gen_key(u, c), kc = fid_hist_gen_key(u, r);
                        rgk = kr < rgk ? kr : rgk;
                        cgk[ni] = kc < cgk[ni] ? kc : cgk[ni];
                    }
                }
                hist_add<PEEL>(h, idx, lane);
            }
            // the row's keys over the 16 lanes of the lane group that share it; genuine pairs are rare: their reduction only where there is one
            if (__ballot(rik != 0ull) != 0) {               // (wave-uniform)
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { const u64 k = shfl_xor_u64(rik, o); rik = k > rik ? k : rik; }
                if ((lane & 15) == 0 && rik != 0ull) atomicMax(a.ikey + r, rik);       // (a key names a pair: the row is < its column < n)
            }
            if (__ballot(rgk != ~0ull) != 0) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { const u64 k = shfl_xor_u64(rgk, o); rgk = k < rgk ? k : rgk; }
                if ((lane & 15) == 0 && rgk != ~0ull) atomicMin(a.gkey + r, rgk);
            }
        }
#pragma unroll
    for (int ni = 0; ni < HNI; ni++) {
        if (__ballot(cik[ni] != 0ull) != 0) {               // (wave-uniform)
            u64 k = shfl_xor_u64(cik[ni], 16);
            cik[ni] = k > cik[ni] ? k : cik[ni];
            k = shfl_xor_u64(cik[ni], 32);
            cik[ni] = k > cik[ni] ? k : cik[ni];
            if ((lane >> 4) == 0 && cik[ni] != 0ull) atomicMax(a.ikey + c0 + ni * 16, cik[ni]);        // (a column with a key: it is < n)
        }
        if (__ballot(cgk[ni] != ~0ull) != 0) {
            u64 k = shfl_xor_u64(cgk[ni], 16);
            cgk[ni] = k < cgk[ni] ? k : cgk[ni];
            k = shfl_xor_u64(cgk[ni], 32);
            cgk[ni] = k < cgk[ni] ? k : cgk[ni];
            if ((lane >> 4) == 0 && cgk[ni] != ~0ull) atomicMin(a.gkey + c0 + ni * 16, cgk[ni]);
        }
    }
    if (__ballot(non_finite != 0u) != 0) {                  // (wave-uniform; rows with an inf or a NaN element only)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) non_finite += (unsigned)__shfl_xor((int)non_finite, o);
        if (lane == 0) atomicAdd(a.summary + 3, (u64)non_finite);
    }
}

// the workgroup's LDS counters into hist_dev, non-zero ones only, and back to zero
__device__ __forceinline__ void hist_flush(const HArgs &a, unsigned *h, int tid) {
    for (int i = tid; i < 2 * a.bins; i += 256) {
        const unsigned v = h[i];
        if (v) {
            atomicAdd(a.hist + i, (u64)v);
            h[i] = 0u;
        }
    }
}

// a workgroup takes every gridDim.x-th place: ascending, so its super-tiles come one after the other and a change of super-tile is the
// moment to flush.  The last K-step's barrier of a tile pair is also the one that frees the LDS tile buffers for the next pair.
template <int PEEL>
__global__ void __launch_bounds__(256) hist_pass(const HArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *h = (unsigned *)(smem + HTILE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 2 * a.bins; i += 256) h[i] = 0u;
    __syncthreads();
    const unsigned per = (unsigned)(a.sw * a.sw);
    u64 cur = 0;
    bool dirty = false;
    for (u64 b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        const u64 sid = b / per;
        const int loc = (int)(b - sid * per);
        // upper triangle of super-tiles, column by column: sid = sg (sg + 1) / 2 + sq with sq <= sg
        long long sg = (long long)((sqrt(8.0 * (double)sid + 1.0) - 1.0) * 0.5);
        while ((u64)sg * (sg + 1) / 2 > sid) sg--;
        while ((u64)(sg + 1) * (sg + 2) / 2 <= sid) sg++;
        const long long sq = (long long)(sid - (u64)sg * (sg + 1) / 2);
        const int ti = (int)sq * a.sw + loc % a.sw, tj = (int)sg * a.sw + loc / a.sw;
        // (the ragged last super-tiles, and the lower half of a diagonal one: no such tile pair -- block-uniform, before any barrier)
        if (ti >= a.n_t || tj >= a.n_t || tj < ti) continue;
        if (dirty && sid != cur) {                          // (block-uniform)
            __syncthreads();                                // every wave's counts of the super-tile before are in
            hist_flush(a, h, tid);                          // (the next counts come behind the barriers of the tile code below)
            dirty = false;
        }
        cur = sid;
        f32x4 acc[HMI][HNI];
        tile_gemm(a, ti * HT, tj * HT, smem, tid, lane, wave & 1, wave >> 1, acc);
        tile_epilogue<PEEL>(a, acc, h, ti, tj, lane, wave & 1, wave >> 1);
        dirty = true;
    }
    if (dirty) {
        __syncthreads();
        hist_flush(a, h, tid);
    }
}

// one thread per position; the first workgroup also adds the class totals up (nobody writes hist any more: behind the kernel boundary)
__global__ void __launch_bounds__(256) hist_finish(const HArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool part = false;
    if (k < a.n) {
        part = a.eff[k] >= 0;
        const u64 ik = a.ikey[k], gk = a.gkey[k];
        const bool hi = part && ik != 0ull, hg = part && gk != ~0ull;
        a.imp_via[k] = hi ? (int)~(unsigned)ik : -1;
        a.imp_score[k] = hi ? __uint_as_float(fid_hist_unsortable((unsigned)(ik >> 32))) : 0.f;
        a.eff[k] = hg ? (int)(unsigned)gk : -1;             // gen_via: the effective label has done its work
        a.gen_score[k] = hg ? __uint_as_float(fid_hist_unsortable((unsigned)(gk >> 32))) : 0.f;
    }
    const int c = __popcll(__ballot(part));
    if (lane == 0 && c) atomicAdd(a.summary + 0, (u64)c);
    if (blockIdx.x == 0) {
#pragma unroll
        for (int cls = 0; cls < 2; cls++) {
            u64 t = 0;
            for (int i = threadIdx.x; i < a.bins; i += 256) t += a.hist[(size_t)cls * a.bins + i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += shfl_xor_u64(t, o);
            if (lane == 0 && t) atomicAdd(a.summary + 1 + cls, t);
        }
    }
}

}  // namespace
}  // namespace fid

extern "C" {

int fid_gallery_score_hist(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const int32_t *labels_dev, int n, int bins, uint64_t *hist_dev,
                           int32_t *imp_via_dev, float *imp_score_dev, int32_t *gen_via_dev, float *gen_score_dev, uint64_t *summary_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && labels_dev && hist_dev && imp_via_dev && imp_score_dev && gen_via_dev && gen_score_dev && summary_dev,
                "score_hist: NULL context, gallery, labels or output pointer");
    FID_REQUIRE(((uintptr_t)hist_dev & 7) == 0 && ((uintptr_t)summary_dev & 7) == 0, "score_hist: hist_dev and summary_dev must be 8-byte aligned");
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    if (!rows_dev) n = G;
    FID_REQUIRE(n > 0 && n <= FID_HIST_MAX_ROWS, "score_hist: %d rows (1 .. %d per call)", n, FID_HIST_MAX_ROWS);
    FID_REQUIRE(bins >= 2 && bins <= FID_HIST_MAX_BINS && bins % 2 == 0, "score_hist: %d bins (an even count, 2 .. %d)", bins, FID_HIST_MAX_BINS);
    FID_REQUIRE(dim > 0 && dim % HCK == 0, "score_hist: embedding dim %d must be a multiple of %d", dim, HCK);
    FID_REQUIRE((size_t)Gp * dim * 2 + (size_t)HT * dim * 2 < 0xFFFFFF00ull, "score_hist: gallery larger than 4 GiB");
    HArgs a{};
    a.n_t = cdiv(n, HT);
    a.sw = std::min(HSUPER, a.n_t);
    const long long n_s = cdiv(a.n_t, a.sw);
    a.blocks = (u64)(n_s * (n_s + 1) / 2) * (unsigned)(a.sw * a.sw);
    // FID_HIST_PEEL (0 or 4) and FID_HIST_GRID (workgroups of the pass) are read per call: measurements; the answer depends on neither
    int peel = 0;
    if (const char *e = getenv("FID_HIST_PEEL")) peel = atoi(e);
    FID_REQUIRE(peel == 0 || peel == 4, "score_hist: FID_HIST_PEEL=%d (0 or 4)", peel);
    // a workgroup keeps its LDS histogram over all its tile pairs of a super-tile: a fixed grid of eight workgroups per CU, each walking many places
    long long want = (long long)ctx->num_cus * 8;
    if (const char *e = getenv("FID_HIST_GRID")) want = atoll(e);
    FID_REQUIRE(want >= 1, "score_hist: FID_HIST_GRID=%lld must be >= 1", want);
    const unsigned grid = (unsigned)std::min<u64>(a.blocks, (u64)std::min<long long>(want, 1ll << 20));
    const int lds = HTILE_BYTES + 2 * bins * (int)sizeof(unsigned);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // scratch slot 2 (shared with fid_match / fid_gallery_group / fid_gallery_dedup / fid_gallery_cluster; calls are serialised by the context's
    // mutex and ordered by its stream): 16 bytes per position, laid out for n rounded up to 65 536 so that the arena is replaced (behind a stream
    // synchronise, the rule of get_scratch) at most when a call crosses such a step
    const size_t ncap = ((size_t)n + 65535) & ~(size_t)65535;
    void *ws;
    FID_TRY(get_scratch(ctx, 2, ncap * 16, &ws));
    const void *fn = peel == 0 ? (const void *)hist_pass<0> : (const void *)hist_pass<4>;
    FID_TRY(ensure_dyn_lds(ctx, fn, lds));
    a.gal = rows; a.rows = rows_dev; a.labels = labels_dev;
    a.ikey = (u64 *)ws;
    a.gkey = (u64 *)ws + ncap;
    a.hist = (u64 *)hist_dev; a.summary = (u64 *)summary_dev;
    a.imp_via = imp_via_dev; a.eff = gen_via_dev; a.imp_score = imp_score_dev; a.gen_score = gen_score_dev;
    a.bins = bins; a.n = n; a.G = G; a.dim = dim;
    a.g_bytes = (unsigned)((size_t)Gp * dim * 2);
    hipLaunchKernelGGL(hist_prepare, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a);
    if (peel == 0) hipLaunchKernelGGL(hist_pass<0>, dim3(grid), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(hist_pass<4>, dim3(grid), dim3(256), lds, ctx->stream, a);
    hipLaunchKernelGGL(hist_finish, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_score_hist_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, int n, int bins, uint64_t *hist,
                        int32_t *imp_via, float *imp_score, int32_t *gen_via, float *gen_score, uint64_t *summary) {
    if (!rows && rows_f16) n = G;
    const char *why = fid_score_hist_check(rows_f16, G, dim, labels, n, bins, hist, imp_via, imp_score, gen_via, gen_score, summary);
    FID_REQUIRE(why == nullptr, "score_hist host: %s", why ? why : "");
    FID_REQUIRE(n <= FID_HIST_MAX_ROWS, "score_hist host: %d rows (1 .. %d per call)", n, FID_HIST_MAX_ROWS);
    fid_score_hist_table_host(rows_f16, G, dim, rows, labels, n, bins, hist, imp_via, imp_score, gen_via, gen_score, summary);
    return FID_OK;
}

}  // extern "C"
