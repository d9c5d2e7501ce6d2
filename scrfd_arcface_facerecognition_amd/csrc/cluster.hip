// Density clusters of stored faces, order-free: "which of these n faces are the same person" as ONE asynchronous call whose answer does not
// depend on the order of the rows (include/faceid.h has the rule in full; tests/cluster_oracle.py is its executable form).
//
//     hit(j, k)  = the rule of fid_gallery_range: fp32 cosine of the two stored fp16 rows >= thresh and > 0
//     degree[k]  = 1 + the other positions that hit k;  core[k] = degree[k] >= min_pts (DBSCAN's min_samples: the point itself counts)
//     cluster    = a connected component of the hit graph restricted to cores; its label is its LOWEST core position
//     via[k]     = the core c != k that hits k with the highest score (lowest position among equal scores); a non-core position with a via
//                  is a border and takes via's label.  That is a rule: sklearn's DBSCAN gives a border point to whichever cluster reaches
//                  it first.
//
// Launch chain on the context's stream: prepare, degree pass, link pass, finish.  Order comes ONLY from stream order: no workgroup waits
// for another one, no flag is polled, nothing is launched cooperatively (the discipline of dedup.hip).
//
//   cluster_prepare  one wave per position: takes part (row inside the gallery, a non-zero element; the sign bit does not count) ->
//                    degree = 1 or 0, parent[k] = k, key[k] = 0.
//   cluster_pass<0>  the degree pass: the upper triangle of 128 x 128 position tiles, diagonal tiles included, only pairs i < j; walked
//                    super-tile by super-tile (range_join.hip), operands read THROUGH rows[] by dedup.hip's tile code (register-staged
//                    buffer loads, a plain LDS double buffer, one __syncthreads() per K-step, no hand-counted waits).  The epilogue counts
//                    the hits per row and per column of the wave's 64 x 64 part, reduces inside the wave (rows: the 16 lanes of a lane
//                    group; columns: registers and the four lane groups; four byte counters per shuffled word) and issues ONE integer
//                    atomicAdd per position and wave: integer sums do not depend on the arrival order.  A tile pair with a hit sets its
//                    bit in the tile-pair bitmap.
//   cluster_pass<1>  the link pass: the same walk, tile pairs whose bit is clear skipped.  The same tile code in the same K order, and one
//                    tile alone computes a given pair: its hit decisions are the degree pass's.  core is final now.  A hit between two
//                    cores is hooked (lock-free union-find: the larger root is hung under the smaller one by atomicCAS, so the root of a
//                    component is its lowest position whatever the arrival order; paths are shortened by atomicMin).  Every read of a
//                    parent word in this kernel is a relaxed agent-scope atomic load, never a plain one: a stale line from another XCD
//                    must not be trusted.  A hit whose other side is a core raises the position's key score bits << 32 | ~core by a 64-bit
//                    atomicMax, reduced per row and per column inside the wave first (dedup_cross): one atomic per position and wave.
//   cluster_finish   one thread per position: the root by following parents (nobody writes them any more), label / via / score, the
//                    summary from per-wave counts and one integer atomic each.
//
// Every hook and find loop is bounded by n + 1 iterations.  Paths only ever lead to lower positions, so a correct run never gets there; a
// loop that does stops and sets summary[5] (the Python layer raises).  A seat belt, not a code path.
// No n x n matrix and no pair list exists anywhere; the gallery is never written.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "cluster_core.h"
#include "common.h"

namespace fid {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int CT = 128, CCK = 32;                         // tile edge in positions, K-step
constexpr int CMI = 4, CNI = 4;                           // fragments of a wave: 64 x 64
constexpr int COP_BYTES = CT * CCK * 2;                   // 8 KB per operand and step
constexpr unsigned COOB = 0xFFFFFF00u;                    // past the gallery (checked to be smaller): such a load returns zeros
constexpr int CSUPER = 16;                                // super-tile edge in tiles (range_join.hip)

struct CLArgs {
    void *gal;                                            // [Gp][dim] unit fp16, read only
    const int32_t *rows;                                  // [n] gallery row of every position, or NULL: position k is row k
    int32_t *parent;                                      // [n]
    u64 *keys;                                            // [n]
    unsigned *bitmap;                                     // bit tj (tj + 1) / 2 + ti: tile pair (ti <= tj) holds a hit
    int32_t *label, *degree, *via, *summary;
    float *score;
    float thresh;
    int min_pts, n, G, dim, n_t, sw, skip;
    u64 blocks;                                           // places of all super-tiles; a workgroup takes every gridDim.x-th one
    unsigned g_bytes;
};

__device__ __forceinline__ bool is_hit(float s, float thresh) { return s >= thresh && s > 0.f; }      // (a NaN fails both)
__device__ __forceinline__ int row_of(const CLArgs &a, int pos) { return a.rows ? a.rows[pos] : pos; }

// dedup.hip's tile_gemm: positions pos_a .. + 127 x positions pos_b .. + 127 (a position >= n or with a row outside the gallery reads as zeros):
// acc[mi][ni][j] = position (pos_a + 64 wm + 16 mi + 4 (lane >> 4) + j) x position (pos_b + 64 wn + 16 ni + (lane & 15)).  Ends behind a barrier.
__device__ __forceinline__ void tile_gemm(const CLArgs &a, int pos_a, int pos_b, char *smem, int tid, int lane, int wm, int wn,
                                          f32x4 (&acc)[CMI][CNI]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.gal, 0, a.g_bytes, 0x00020000);
    const unsigned rowb = (unsigned)a.dim * 2u;
    const int lrow = tid >> 2, lgrp = tid & 3;
    unsigned a_src[2], b_src[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int pa = pos_a + lrow + 64 * i, pb = pos_b + lrow + 64 * i;
        const int ra = pa < a.n ? row_of(a, pa) : -1, rb = pb < a.n ? row_of(a, pb) : -1;
        a_src[i] = (ra >= 0 && ra < a.G) ? (unsigned)ra * rowb + (unsigned)lgrp * 16u : COOB;
        b_src[i] = (rb >= 0 && rb < a.G) ? (unsigned)rb * rowb + (unsigned)lgrp * 16u : COOB;
    }
    const int st_off = lrow * 64 + ((lgrp ^ ((lrow >> 1) & 3)) * 16);
    u32x4 ra[2], rb[2];
    auto issue_loads = [&](int ks) {
        const unsigned kb = (unsigned)ks * (CCK * 2);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, a_src[i] != COOB ? a_src[i] + kb : COOB, 0, 0);
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, b_src[i] != COOB ? b_src[i] + kb : COOB, 0, 0);
        }
    };
    auto store_tiles = [&](int buf) {
        char *dst = smem + buf * 2 * COP_BYTES + st_off;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *(u32x4 *)(dst + i * 64 * 64) = ra[i];
            *(u32x4 *)(dst + COP_BYTES + i * 64 * 64) = rb[i];
        }
    };
#pragma unroll
    for (int mi = 0; mi < CMI; mi++)
#pragma unroll
        for (int ni = 0; ni < CNI; ni++) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = a.dim / CCK;
    issue_loads(0);
    store_tiles(0);
    __syncthreads();
    const int frow = lane & 15, fq = lane >> 4;
    const int grp = (fq ^ ((frow >> 1) & 3)) * 16;
    const int a_off = (wm * 64 + frow) * 64 + grp, b_off = COP_BYTES + (wn * 64 + frow) * 64 + grp;
    for (int ks = 0; ks < ksteps; ks++) {
        const int cur = ks & 1;
        const bool more = ks + 1 < ksteps;
        if (more) issue_loads(ks + 1);
        const char *st = smem + cur * 2 * COP_BYTES;
        half8 af[CMI], bf[CNI];
#pragma unroll
        for (int mi = 0; mi < CMI; mi++) af[mi] = *(const half8 *)(st + a_off + mi * 1024);
#pragma unroll
        for (int ni = 0; ni < CNI; ni++) bf[ni] = *(const half8 *)(st + b_off + ni * 1024);
#pragma unroll
        for (int mi = 0; mi < CMI; mi++)
#pragma unroll
            for (int ni = 0; ni < CNI; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        if (more) store_tiles(cur ^ 1);                     // last read in step ks - 1, behind that step's barrier
        __syncthreads();
    }
}

// one wave per position: does it take part?  Also the per-call state of the position.
__global__ void __launch_bounds__(256) cluster_prepare(const CLArgs a) {
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
        a.degree[pos] = any != 0u;
        a.parent[pos] = pos;
        a.keys[pos] = 0ull;
    }
}

__device__ __forceinline__ int parent_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's tree, by relaxed agent-scope atomic loads; -1 when the bound is reached (never in a correct run: a path leads to ever
// lower positions).  The start of a path longer than one step is hung nearer the root: an ancestor replaces an ancestor.
__device__ __forceinline__ int find_root(const CLArgs &a, int v) {
    const int start = v;
    int p = parent_load(a.parent + v), steps = 0;
    for (int it = 0; p != v; it++) {
        if (it > a.n) return -1;
        v = p;
        p = parent_load(a.parent + v);
        steps++;
    }
    if (steps > 1) atomicMin(a.parent + start, v);
    return v;
}

// union of the trees of u and v: the larger root is hung under the smaller one.  false: the bound was reached.
__device__ __forceinline__ bool hook(const CLArgs &a, int u, int v) {
    for (int it = 0; it <= a.n; it++) {
        u = find_root(a, u);
        v = find_root(a, v);
        if (u < 0 || v < 0) return false;
        if (u == v) return true;
        if (u > v) { const int t = u; u = v; v = t; }
        const int old = atomicCAS(a.parent + v, v, u);      // v is hung only while it still is a root
        if (old == v) return true;
        v = old;                                            // somebody hung v first, under a lower position: go on from there
    }
    return false;
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 k, int o) {
    return ((u64)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), o) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, o);
}

// one tile pair: linear id b -> (ti, tj) of the upper triangle, walked super-tile by super-tile as in range_join.hip
template <int LINK>
__device__ __forceinline__ void tile_pair(const CLArgs &a, u64 b, char *smem, int tid, int lane, int wm, int wn) {
    const unsigned per = (unsigned)(a.sw * a.sw);
    const u64 sid = b / per;
    const int loc = (int)(b - sid * per);
    // upper triangle of super-tiles, column by column: sid = sg (sg + 1) / 2 + sq with sq <= sg
    long long sg = (long long)((sqrt(8.0 * (double)sid + 1.0) - 1.0) * 0.5);
    while ((u64)sg * (sg + 1) / 2 > sid) sg--;
    while ((u64)(sg + 1) * (sg + 2) / 2 <= sid) sg++;
    const long long sq = (long long)(sid - (u64)sg * (sg + 1) / 2);
    const int ti = (int)sq * a.sw + loc % a.sw, tj = (int)sg * a.sw + loc / a.sw;
    // (the ragged last super-tiles, and the lower half of a diagonal one: no such tile pair -- block-uniform, before any barrier)
    if (ti >= a.n_t || tj >= a.n_t || tj < ti) return;
    const u64 bit = (u64)tj * (tj + 1) / 2 + ti;
    if (LINK && a.skip && !((a.bitmap[bit >> 5] >> (bit & 31)) & 1u)) return;        // (block-uniform; written by the launch before)

    f32x4 acc[CMI][CNI];
    tile_gemm(a, ti * CT, tj * CT, smem, tid, lane, wm, wn, acc);
    const int r0 = ti * CT + wm * 64 + (lane >> 4) * 4, c0 = tj * CT + wn * 64 + (lane & 15);
    // this lane's hits, bit 16 mi + 4 ni + j: row r0 + 16 mi + j x column c0 + 16 ni (only row < column: every unordered pair once)
    u64 mask = 0;
#pragma unroll
    for (int mi = 0; mi < CMI; mi++)
#pragma unroll
        for (int ni = 0; ni < CNI; ni++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = r0 + mi * 16 + j, c = c0 + ni * 16;
                mask |= (u64)(is_hit(acc[mi][ni][j], a.thresh) && r < c && c < a.n) << (mi * 16 + ni * 4 + j);
            }
    if (__ballot(mask != 0) == 0) return;                   // (wave-uniform; no barrier follows)

    if (!LINK) {
        // rows: word mi holds the four byte counters j = 0 .. 3 (at most 4 per lane, 64 per lane group)
        unsigned rw[CMI];
#pragma unroll
        for (int mi = 0; mi < CMI; mi++) {
            rw[mi] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) rw[mi] |= (unsigned)__popcll(mask & (0x1111ull << (mi * 16 + j))) << (8 * j);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) rw[mi] += (unsigned)__shfl_xor((int)rw[mi], o);
        }
        // columns: one word holds the four byte counters ni = 0 .. 3 (at most 16 per lane, 64 per column)
        unsigned cw = 0;
#pragma unroll
        for (int ni = 0; ni < CNI; ni++) cw |= (unsigned)__popcll(mask & (0x000F000F000F000Full << (ni * 4))) << (8 * ni);
        cw += (unsigned)__shfl_xor((int)cw, 16);
        cw += (unsigned)__shfl_xor((int)cw, 32);
        // every lane group holds all counters now: lane l adds for the row mi = (l & 15) >> 2, j = l & 3 of its own group and for the column
        // ni = l >> 4 of its own (l & 15) -- 64 rows and 64 columns on 64 lanes, one atomic per position and wave
        const int t = lane & 15, q = lane >> 4;
        const unsigned w = (t >> 2) == 0 ? rw[0] : (t >> 2) == 1 ? rw[1] : (t >> 2) == 2 ? rw[2] : rw[3];
        const int rcnt = (int)((w >> (8 * (t & 3))) & 255u), r = r0 + (t >> 2) * 16 + (t & 3);
        if (rcnt && r < a.n) atomicAdd(a.degree + r, rcnt);
        const int ccnt = (int)((cw >> (8 * q)) & 255u), c = c0 + q * 16;
        if (ccnt && c < a.n) atomicAdd(a.degree + c, ccnt);
        if (lane == 0) atomicOr(a.bitmap + (bit >> 5), 1u << (bit & 31));
        return;
    }

    // ---- link: core is final (the degree pass ended with the launch before) ----
    bool ccore[CNI];
#pragma unroll
    for (int ni = 0; ni < CNI; ni++) {
        const int c = c0 + ni * 16;
        ccore[ni] = c < a.n && a.degree[c] >= a.min_pts;
    }
    u64 ckey[CNI] = {0ull, 0ull, 0ull, 0ull};
    u64 hooks = 0;                                          // this lane's hits between two cores, by the bits of mask
#pragma unroll
    for (int mi = 0; mi < CMI; mi++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned m4 = (unsigned)(mask >> (mi * 16 + j));          // bits 0, 4, 8, 12: the columns ni
            if (__ballot((m4 & 0x1111u) != 0) == 0) continue;              // (wave-uniform)
            const int r = r0 + mi * 16 + j;
            const bool rcore = r < a.n && a.degree[r] >= a.min_pts;
            u64 rkey = 0;
#pragma unroll
            for (int ni = 0; ni < CNI; ni++) {
                if (!((m4 >> (4 * ni)) & 1u)) continue;
                const int c = c0 + ni * 16;
                const u64 sb = (u64)__float_as_uint(acc[mi][ni][j]) << 32;  // a hit score is > 0: its bits order like the score
                if (ccore[ni]) { const u64 k = sb | (unsigned)~(unsigned)c; rkey = k > rkey ? k : rkey; }
                if (rcore) { const u64 k = sb | (unsigned)~(unsigned)r; ckey[ni] = k > ckey[ni] ? k : ckey[ni]; }
                if (rcore && ccore[ni]) hooks |= 1ull << (mi * 16 + ni * 4 + j);
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { const u64 k = shfl_xor_u64(rkey, o); rkey = k > rkey ? k : rkey; }
            if ((lane & 15) == 0 && rkey) atomicMax(a.keys + r, rkey);      // (a hit row is < its column < n)
        }
#pragma unroll
    for (int ni = 0; ni < CNI; ni++) {
        if (__ballot(ckey[ni] != 0) == 0) continue;                         // (wave-uniform)
        u64 k = shfl_xor_u64(ckey[ni], 16);
        ckey[ni] = k > ckey[ni] ? k : ckey[ni];
        k = shfl_xor_u64(ckey[ni], 32);
        ckey[ni] = k > ckey[ni] ? k : ckey[ni];
        if ((lane >> 4) == 0 && ckey[ni]) atomicMax(a.keys + c0 + ni * 16, ckey[ni]);      // (a column with a key hit: it is < n)
    }
    bool fault = false;
    while (hooks) {                                         // (one copy of the union-find loops, not one per fragment element)
        const int bit = __ffsll((long long)hooks) - 1;
        hooks &= hooks - 1;
        fault |= !hook(a, r0 + (bit >> 4) * 16 + (bit & 3), c0 + ((bit >> 2) & 3) * 16);
    }
    if (fault) atomicOr(a.summary + 5, 1);
}

// a workgroup takes every gridDim.x-th place; the last K-step's barrier is also the one that frees the LDS buffers for the next pair
template <int LINK>
__global__ void __launch_bounds__(256) cluster_pass(const CLArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * COP_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (u64 b = blockIdx.x; b < a.blocks; b += gridDim.x) tile_pair<LINK>(a, b, smem, tid, lane, wave & 1, wave >> 1);
}

// one thread per position.  Nobody writes a parent any more: plain loads, behind the kernel boundary.
__global__ void __launch_bounds__(256) cluster_finish(const CLArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool part = false, core = false, border = false, noise = false, head = false, fault = false;
    if (k < a.n) {
        const int deg = a.degree[k];
        part = deg > 0;
        core = deg >= a.min_pts;                            // (min_pts >= 1: a core takes part)
        const u64 key = a.keys[k];
        const int via = key ? (int)~(unsigned)key : -1;
        int label = -1;
        if (core || (part && via >= 0)) {
            int v = core ? k : via, it = 0;
            for (int p = a.parent[v]; p != v; p = a.parent[v]) {
                if (++it > a.n) { fault = true; break; }
                v = p;
            }
            label = fault ? -1 : v;
        }
        border = part && !core && via >= 0;
        noise = part && !core && via < 0;
        head = core && label == k;
        a.label[k] = label;
        a.via[k] = part ? via : -1;
        a.score[k] = part && key ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
    }
    const bool flags[6] = {head, core, border, noise, part, fault};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const int c = __popcll(__ballot(flags[i]));
        if (lane == 0 && c) { if (i < 5) atomicAdd(a.summary + i, c); else atomicOr(a.summary + 5, 1); }
    }
}

}  // namespace
}  // namespace fid

extern "C" {

int fid_gallery_cluster(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, int n, float thresh, int min_pts, int32_t *label_dev,
                        int32_t *degree_dev, int32_t *via_dev, float *score_dev, int32_t *summary_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && label_dev && degree_dev && via_dev && score_dev && summary_dev, "cluster: NULL context, gallery or output pointer");
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    if (!rows_dev) n = G;
    FID_REQUIRE(n > 0 && n <= FID_CLUSTER_MAX_ROWS, "cluster: %d rows (1 .. %d per call)", n, FID_CLUSTER_MAX_ROWS);
    FID_REQUIRE(min_pts >= 1, "cluster: min_pts %d must be >= 1 (it counts the point itself)", min_pts);
    FID_REQUIRE(!std::isnan(thresh), "cluster: the threshold is NaN");
    FID_REQUIRE(thresh > 0.f, "cluster: threshold %g must be > 0 (a hit needs a score > 0)", thresh);
    FID_REQUIRE(dim > 0 && dim % CCK == 0, "cluster: embedding dim %d must be a multiple of %d", dim, CCK);
    FID_REQUIRE((size_t)Gp * dim * 2 + (size_t)CT * dim * 2 < 0xFFFFFF00ull, "cluster: gallery larger than 4 GiB");
    CLArgs a{};
    a.n_t = cdiv(n, CT);
    a.sw = std::min(CSUPER, a.n_t);
    const long long n_s = cdiv(a.n_t, a.sw);
    a.blocks = (u64)(n_s * (n_s + 1) / 2) * (unsigned)(a.sw * a.sw);
    const unsigned grid = (unsigned)std::min<u64>(a.blocks, 1ull << 20);      // (grid x 256 threads stays below 2^32)
    // FID_CLUSTER_SKIP=0 computes every tile pair again in the link pass (read per call: measurements); the answer does not depend on it
    a.skip = 1;
    if (const char *e = getenv("FID_CLUSTER_SKIP")) a.skip = atoi(e) != 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // scratch slot 2 (shared with fid_match / fid_gallery_group / fid_gallery_dedup; calls are serialised by the context's mutex and ordered by
    // its stream): 12 bytes per position + the tile-pair bitmap, laid out for n rounded up to 65 536 so that the arena is replaced (behind a
    // stream synchronise, the rule of get_scratch) at most when a call crosses such a step
    const size_t ncap = ((size_t)n + 65535) & ~(size_t)65535, tcap = ncap / CT;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_parent = up(ncap * 8), o_bitmap = o_parent + up(ncap * 4), total = o_bitmap + up((tcap * (tcap + 1) / 2 + 31) / 32 * 4);
    void *ws;
    FID_TRY(get_scratch(ctx, 2, total, &ws));
    a.gal = rows; a.rows = rows_dev;
    a.keys = (u64 *)ws;
    a.parent = (int32_t *)((char *)ws + o_parent);
    a.bitmap = (unsigned *)((char *)ws + o_bitmap);
    a.label = label_dev; a.degree = degree_dev; a.via = via_dev; a.score = score_dev; a.summary = summary_dev;
    a.thresh = thresh; a.min_pts = min_pts;
    a.n = n; a.G = G; a.dim = dim;
    a.g_bytes = (unsigned)((size_t)Gp * dim * 2);
    const size_t bitmap_bytes = ((size_t)a.n_t * (a.n_t + 1) / 2 + 31) / 32 * 4;
    FID_HIP(hipMemsetAsync(a.bitmap, 0, bitmap_bytes, ctx->stream));
    FID_HIP(hipMemsetAsync(summary_dev, 0, FID_CLUSTER_SUMMARY_WORDS * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(cluster_prepare, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(cluster_pass<0>, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(cluster_pass<1>, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(cluster_finish, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_cluster_host(const void *rows_f16, int G, int dim, const int32_t *rows, int n, float thresh, int min_pts, int32_t *label, int32_t *degree,
                     int32_t *via, float *score, int32_t *summary) {
    if (!rows && rows_f16) n = G;
    const char *why = fid_cluster_check(rows_f16, G, dim, n, thresh, min_pts, label, degree, via, score, summary);
    FID_REQUIRE(why == nullptr, "cluster host: %s", why ? why : "");
    FID_REQUIRE(n <= FID_CLUSTER_MAX_ROWS, "cluster host: %d rows (1 .. %d per call)", n, FID_CLUSTER_MAX_ROWS);
    fid_cluster_table_host(rows_f16, G, dim, rows, n, thresh, min_pts, label, degree, via, score, summary);
    return FID_OK;
}

}  // extern "C"
