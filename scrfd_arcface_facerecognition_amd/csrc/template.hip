// Identity templates: one gallery row per person from many stored faces, as ONE asynchronous call (include/faceid.h has the rule in full,
// template_core.h the arithmetic, tests/template_oracle.py its executable form).
//
//     member      = a position whose row is inside the gallery, with 0 <= label < P, 1 <= weight <= 255, a non-zero element and every element
//                   finite with |x| <= 2
//     S_pc        = sum of w_k * (x_kc * 2^24) over the members of person p, in int64: exact, so no order of additions can change it
//     template    = S / |S| (the pinned fp64 norm), rounded to fp32 and then to fp16
//     score[k]    = (float)(<X_k, T_p> * 2^-48), the dot product in int64; a member stays when score >= min_score; the final template is the
//                   same rule on the members that stayed
//
// All of it streams rows, so the chain is bound by the bytes it reads.  Order comes ONLY from stream order: no workgroup waits for another one,
// no flag is polled (the discipline of dedup.hip / cluster.hip / calib.hip).  No float atomic anywhere: what is added across waves is integer.
//
//   tpl_prepare   a wave per 64 positions: which of them are members (their rows are read once for the element conditions); the effective label
//                 (or -1) is parked in kept_dev; members per person by integer atomicAdd, one add per wave and distinct label
//   tpl_scan_a/b/c  three exclusive scans over the persons in one go (1024 persons per workgroup: workgroup sums, their scan, the scan inside):
//                 where a person's member list starts, where its CHUNKS start (a chunk = up to `chunk` members = the work of one wave; a person
//                 without a member still has one, which writes its zero row), and its accumulator slot if it has more than one chunk
//   tpl_scatter   the inverted index: position, gallery row and weight of every member into its person's list (the place inside a list is
//                 whatever the atomics hand out: nothing below depends on it)
//   tpl_sum       a wave per chunk, found by bisection in the chunk starts: every lane loads 16 bytes of a row (a 512-wide row is ONE 1 KB wave
//                 load), four rows in flight, and keeps its columns' int64 sums in registers.  A person of one chunk is finished in the same
//                 wave; a split person's chunks add into ITS accumulator row with 64-bit integer atomics, laid out so that one wave
//                 instruction adds 512 contiguous bytes, and tpl_finish (a wave per split person) takes the row from there and clears it.
//                 FID_TEMPLATE_COMBINE=pass (measurements; the default is the atomics) is the second-pass form instead: every chunk of a
//                 split person stores its partial row with plain stores and tpl_finish adds a person's partial rows up.
//   tpl_score     a wave per chunk: the template as integers in registers, every member row against it; score, kept, the weight that stays, and
//                 the person's lowest / highest member as packed keys by 64-bit atomicMin / atomicMax
//   tpl_sum / tpl_finish again on the weights that stayed, for the persons that lost a member only (skipped without trimming)
//   tpl_report    a thread per person: the person words, and the counts of the summary
//
// Scratch: 12 bytes per position and 48 per person, plus one accumulator row of (dim + 8) int64 per person that is actually split -- room for
// n / (chunk + 1) of them, the most there can be (cleared for the split persons only, by tpl_clear; the second-pass form takes a row per chunk
// of a split person instead, at most 2 n / chunk + 1).  No [P, dim] array of sums exists.  The gallery is never written.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "template_core.h"

namespace fid {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
typedef long long i64;

constexpr int SCAN = 1024;                                // persons per workgroup of the scans

struct TArgs {
    const char *gal;                                      // [Gp][dim] fp16, read only
    const int32_t *rows, *labels, *weights;               // [n]; rows / weights may be NULL
    int n, P, G, dim, chunk, keep_all, combine;          // combine: 0 = int64 atomics, 1 = partial rows and a second pass
    float min_score;
    // scratch
    int32_t *count, *start, *cstart, *sslot, *pslot, *cursor, *keptc, *split_person, *bsum, *hdr;
    u64 *klow, *khigh;
    int32_t *lpos, *lrow, *lw, *lwk;
    i64 *acc, *part;                                      // accumulator rows [split persons]; partial rows [chunks of split persons]
    int acc_stride;
    // outputs
    uint16_t *tpl;
    float *score;
    int32_t *kept, *person;
    float *cohesion;
    u64 *summary;
};

enum { HDR_MEMBERS = 0, HDR_CHUNKS = 1, HDR_SPLIT = 2 };

__device__ __forceinline__ u64 shfl_xor_u64(u64 k, int o) {
    return ((u64)(unsigned)__shfl_xor((int)(unsigned)(k >> 32), o) << 32) | (unsigned)__shfl_xor((int)(unsigned)k, o);
}
__device__ __forceinline__ double shfl_xor_f64(double v, int o) { return __longlong_as_double((i64)shfl_xor_u64((u64)__double_as_longlong(v), o)); }

// one count into counter[idx] for every lane with idx >= 0, ONE atomic per distinct idx of the wave (the whole wave calls this together);
// -> the lane's place among all adds to its counter (the value before the wave's add plus its rank inside the wave), -1 for idx < 0
__device__ __forceinline__ int wave_count(int32_t *counter, int idx, int lane) {
    int base = 0, lead_of = lane, rank = 0, todo = idx;
    for (;;) {
        const u64 live = __ballot(todo >= 0);
        if (live == 0) break;                             // (wave-uniform)
        const int lead = __ffsll((i64)live) - 1;
        const int first = __shfl(todo, lead);
        const u64 same = __ballot(todo == first);
        if (todo == first) {
            lead_of = lead;
            rank = __popcll(same & ((1ull << lane) - 1ull));
            if (lane == lead) base = atomicAdd(counter + first, __popcll(same));
            todo = -1;
        }
    }
    const int b = __shfl(base, lead_of);
    return idx >= 0 ? b + rank : -1;
}

// a wave per 64 consecutive positions
__global__ void __launch_bounds__(256) tpl_prepare(const TArgs a) {
    const int lane = threadIdx.x & 63;
    const int p0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (p0 >= a.n) return;                                // (wave-uniform)
    const int pos = p0 + lane;
    int row = -1, label = -1;
    bool elig = false;
    if (pos < a.n) {
        row = a.rows ? a.rows[pos] : pos;
        label = a.labels[pos];
        const int w = a.weights ? a.weights[pos] : 1;
        elig = row >= 0 && row < a.G && label >= 0 && label < a.P && w >= 1 && w <= 255;
    }
    const u64 todo = __ballot(elig);
    const int pieces = a.dim >> 3;                        // 16-byte pieces of a row
    bool ok = false;
    for (int j0 = 0; j0 < 64; j0 += 4) {
        if (((todo >> j0) & 15ull) == 0) continue;        // (wave-uniform)
        unsigned any[4] = {0, 0, 0, 0}, bad[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!((todo >> (j0 + u)) & 1ull)) continue;   // (wave-uniform)
            const u32x4 *src = (const u32x4 *)(a.gal + (size_t)__shfl(row, j0 + u) * a.dim * 2);
            for (int i = lane; i < pieces; i += 64) {
                const u32x4 v = src[i];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const unsigned lo = v[e] & 0x7FFFu, hi = (v[e] >> 16) & 0x7FFFu;
                    any[u] |= lo | hi;
                    bad[u] |= (unsigned)(lo > 0x4000u) | (unsigned)(hi > 0x4000u);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool fine = __ballot(any[u] != 0u) != 0 && __ballot(bad[u] != 0u) == 0;
            if (lane == j0 + u) ok = elig && fine;
        }
    }
    if (pos < a.n) {
        a.kept[pos] = ok ? label : -1;                    // the effective label, until tpl_score writes the decision
        a.score[pos] = 0.f;
    }
    wave_count(a.count, ok ? label : -1, lane);
    const int rejected = __popcll(__ballot(elig && !ok));
    if (lane == 0 && rejected) atomicAdd(a.summary + 4, (u64)rejected);
}

// exclusive scan of v over the 1024 threads of the workgroup; lds: 16 words
__device__ __forceinline__ int block_excl_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int s = lds[i];
        base += i < wave ? s : 0;
        tot += s;
    }
    __syncthreads();                                      // (lds is free for the next scan)
    total = tot;
    return base + inc - v;
}

// what person p brings to the three scans: members, chunks (at least one), 1 if split
__device__ __forceinline__ void person_words(const TArgs &a, int p, int &c, int &nch, int &split, int &parts) {
    c = p < a.P ? a.count[p] : 0;
    nch = p < a.P ? max(1, (c + a.chunk - 1) / a.chunk) : 0;
    split = c > a.chunk;
    parts = split ? nch : 0;                              // the chunks of split persons: the partial rows of the second-pass form
}

__global__ void __launch_bounds__(SCAN) tpl_scan_a(const TArgs a) {
    __shared__ int lds[16];
    int c, nch, split, parts, t0, t1, t2, t3;
    person_words(a, blockIdx.x * SCAN + threadIdx.x, c, nch, split, parts);
    block_excl_scan(c, lds, t0);
    block_excl_scan(nch, lds, t1);
    block_excl_scan(split, lds, t2);
    block_excl_scan(parts, lds, t3);
    if (threadIdx.x == 0) {
        a.bsum[4 * blockIdx.x + 0] = t0;
        a.bsum[4 * blockIdx.x + 1] = t1;
        a.bsum[4 * blockIdx.x + 2] = t2;
        a.bsum[4 * blockIdx.x + 3] = t3;
    }
}

// one workgroup: the sums of the (at most 1024) workgroups of tpl_scan_a become their offsets; the totals
__global__ void __launch_bounds__(SCAN) tpl_scan_b(const TArgs a, int nb) {
    __shared__ int lds[16];
    const int t = threadIdx.x;
    int v[4], tot[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = t < nb ? a.bsum[4 * t + i] : 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = block_excl_scan(v[i], lds, tot[i]);
    if (t < nb) {
#pragma unroll
        for (int i = 0; i < 4; i++) a.bsum[4 * t + i] = v[i];
    }
    if (t == 0) {
        a.hdr[HDR_MEMBERS] = tot[0];
        a.hdr[HDR_CHUNKS] = tot[1];
        a.hdr[HDR_SPLIT] = tot[2];
        a.start[a.P] = tot[0];
        a.cstart[a.P] = tot[1];
        a.summary[0] = (u64)tot[0];
    }
}

__global__ void __launch_bounds__(SCAN) tpl_scan_c(const TArgs a) {
    __shared__ int lds[16];
    const int p = blockIdx.x * SCAN + threadIdx.x;
    int c, nch, split, parts, tot;
    person_words(a, p, c, nch, split, parts);
    const int s0 = block_excl_scan(c, lds, tot) + a.bsum[4 * blockIdx.x + 0];
    const int s1 = block_excl_scan(nch, lds, tot) + a.bsum[4 * blockIdx.x + 1];
    const int s2 = block_excl_scan(split, lds, tot) + a.bsum[4 * blockIdx.x + 2];
    const int s3 = block_excl_scan(parts, lds, tot) + a.bsum[4 * blockIdx.x + 3];
    if (p >= a.P) return;
    a.pslot[p] = s3;                                      // (s3 + nch <= the chunks of all split persons <= 2 n / chunk)
    a.start[p] = s0;
    a.cstart[p] = s1;
    a.sslot[p] = split ? s2 : -1;
    if (split) a.split_person[s2] = p;                    // (s2 < the number of split persons <= n / (chunk + 1))
    a.cursor[p] = 0;
    a.keptc[p] = 0;
    a.klow[p] = ~0ull;
    a.khigh[p] = 0ull;
}

// a wave per accumulator row that a split person will use: zeroed here, so a call clears what it needs and not the whole area
__global__ void __launch_bounds__(256) tpl_clear(const TArgs a) {
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.hdr[HDR_SPLIT]) return;
    i64 *row = a.acc + (size_t)s * a.acc_stride;
    for (int i = lane; i < a.acc_stride; i += 64) row[i] = 0;
}

// a thread per position: members go into their person's list
__global__ void __launch_bounds__(256) tpl_scatter(const TArgs a) {
    const int pos = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int label = pos < a.n ? a.kept[pos] : -1;
    const int at = wave_count(a.cursor, label, lane);
    if (label >= 0) {
        const int slot = a.start[label] + at;             // (at < count[label]: the same positions were counted by tpl_prepare)
        a.lpos[slot] = pos;
        a.lrow[slot] = a.rows ? a.rows[pos] : pos;
        a.lw[slot] = a.weights ? a.weights[pos] : 1;
    }
}

// the chunk of wave w: -> person, its first and one-past-last list slot, the number of chunks of the person; false = no such chunk
__device__ __forceinline__ bool chunk_of(const TArgs &a, int w, int &p, int &m0, int &m1, int &nch, int &j) {
    if (w >= a.hdr[HDR_CHUNKS]) return false;
    int lo = 0, hi = a.P - 1;
    while (lo < hi) {                                     // the last person whose chunks start at or before w (every person has a chunk)
        const int mid = (lo + hi + 1) >> 1;
        if (a.cstart[mid] <= w) lo = mid; else hi = mid - 1;
    }
    p = lo;
    const int first = a.cstart[p], s = a.start[p], e = a.start[p + 1];
    nch = a.cstart[p + 1] - first;
    j = w - first;
    m0 = min(e, s + j * a.chunk);
    m1 = min(e, m0 + a.chunk);
    return true;
}

// the lane's place for column block blk, element e in an accumulator row: one wave instruction touches 512 contiguous bytes
__device__ __forceinline__ int acc_at(int blk, int e, int lane) { return blk * 512 + e * 64 + lane; }

// norm, template row, cohesion of person p from the sums in registers (lane l holds columns blk * 512 + l * 8 + e)
template <int NB>
__device__ __forceinline__ void finalize(const TArgs &a, const i64 (&S)[NB][8], i64 W, int p, int lane) {
    double v = 0.0;
#pragma unroll
    for (int blk = 0; blk < NB; blk++)
#pragma unroll
        for (int e = 0; e < 8; e++) {                     // (sums of columns at or beyond dim are zero: + 0.0 changes nothing)
            const double d = (double)S[blk][e];
            const double q = d * d;
            v = v + q;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + shfl_xor_f64(v, o);
    const double nrm = sqrt(v);
#pragma unroll
    for (int blk = 0; blk < NB; blk++) {
        const int c0 = blk * 512 + lane * 8;
        if (c0 < a.dim) {
            unsigned h[8];
#pragma unroll
            for (int e = 0; e < 8; e++) h[e] = nrm > 0.0 ? (unsigned)fid_tpl_f32_to_f16(fid_tpl_element(S[blk][e], nrm)) : 0u;
            u32x4 out = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            *(u32x4 *)(a.tpl + (size_t)p * a.dim + c0) = out;
        }
    }
    if (lane == 0) a.cohesion[p] = fid_tpl_cohesion(nrm, W);
}

__device__ __forceinline__ void unpack8(const u32x4 v, int32_t (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        x[2 * e] = fid_tpl_fixed((uint16_t)(v[e] & 0xFFFFu));
        x[2 * e + 1] = fid_tpl_fixed((uint16_t)(v[e] >> 16));
    }
}

// a wave per chunk.  PHASE 0: every member at its weight.  PHASE 1: the weights that stayed, persons that lost a member only.
template <int NB, int PHASE>
__global__ void __launch_bounds__(256) tpl_sum(const TArgs a) {
    const int lane = threadIdx.x & 63;
    int p, m0, m1, nch, j;
    if (!chunk_of(a, blockIdx.x * 4 + (threadIdx.x >> 6), p, m0, m1, nch, j)) return;       // (wave-uniform, like everything below)
    if (PHASE == 1 && a.keptc[p] == a.count[p]) return;
    const int32_t *wsrc = PHASE == 0 ? a.lw : a.lwk;
    i64 S[NB][8];
#pragma unroll
    for (int blk = 0; blk < NB; blk++)
#pragma unroll
        for (int e = 0; e < 8; e++) S[blk][e] = 0;
    i64 W = 0;
    const int pieces = a.dim >> 3;
    for (int b = m0; b < m1; b += 64) {
        const int idx = b + lane, cnt = min(64, m1 - b);
        const int myrow = idx < m1 ? a.lrow[idx] : 0, myw = idx < m1 ? wsrc[idx] : 0;
        for (int i0 = 0; i0 < cnt; i0 += 4) {
            u32x4 v[4][NB];
            int w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {                 // (lanes at or beyond cnt hold weight 0)
                w[u] = __shfl(myw, (i0 + u) & 63);
                const u32x4 *src = (const u32x4 *)(a.gal + (size_t)__shfl(myrow, (i0 + u) & 63) * a.dim * 2);
#pragma unroll
                for (int blk = 0; blk < NB; blk++) {
                    const int piece = blk * 64 + lane;
                    v[u][blk] = (w[u] != 0 && piece < pieces) ? src[piece] : u32x4{0u, 0u, 0u, 0u};
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int blk = 0; blk < NB; blk++) {
                    int32_t x[8];
                    unpack8(v[u][blk], x);
#pragma unroll
                    for (int e = 0; e < 8; e++) S[blk][e] += (i64)w[u] * (i64)x[e];
                }
                W += w[u];
            }
        }
    }
    if (nch == 1) {
        finalize<NB>(a, S, W, p, lane);
        return;
    }
    if (a.combine) {                                      // the chunk's partial row, every word of it, with plain stores
        i64 *mine = a.part + (size_t)(a.pslot[p] + j) * a.acc_stride;
#pragma unroll
        for (int blk = 0; blk < NB; blk++)
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (blk * 512 + lane * 8 < a.dim) mine[acc_at(blk, e, lane)] = S[blk][e];
        if (lane == 0) mine[NB * 512] = W;
        return;
    }
    i64 *row = a.acc + (size_t)a.sslot[p] * a.acc_stride;
#pragma unroll
    for (int blk = 0; blk < NB; blk++)
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (blk * 512 + lane * 8 < a.dim && S[blk][e] != 0) atomicAdd((u64 *)row + acc_at(blk, e, lane), (u64)S[blk][e]);
    if (lane == 0 && W != 0) atomicAdd((u64 *)row + NB * 512, (u64)W);
}

// a wave per split person: its accumulator row into registers (and back to zero, for the next pass and the next call)
template <int NB, int PHASE>
__global__ void __launch_bounds__(256) tpl_finish(const TArgs a) {
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.hdr[HDR_SPLIT]) return;
    const int p = a.split_person[s];
    if (PHASE == 1 && a.keptc[p] == a.count[p]) return;
    i64 S[NB][8];
    if (a.combine) {                                      // the second pass: the partial rows of the person's chunks, added up
#pragma unroll
        for (int blk = 0; blk < NB; blk++)
#pragma unroll
            for (int e = 0; e < 8; e++) S[blk][e] = 0;
        i64 W = 0;
        const int nch = a.cstart[p + 1] - a.cstart[p];
        const i64 *first = a.part + (size_t)a.pslot[p] * a.acc_stride;
        for (int j = 0; j < nch; j++) {
            const i64 *r = first + (size_t)j * a.acc_stride;
#pragma unroll
            for (int blk = 0; blk < NB; blk++)
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (blk * 512 + lane * 8 < a.dim) S[blk][e] += r[acc_at(blk, e, lane)];
            W += r[NB * 512];
        }
        finalize<NB>(a, S, W, p, lane);
        return;
    }
    i64 *row = a.acc + (size_t)s * a.acc_stride;
#pragma unroll
    for (int blk = 0; blk < NB; blk++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const bool in = blk * 512 + lane * 8 < a.dim;
            S[blk][e] = in ? row[acc_at(blk, e, lane)] : 0;
            if (in) row[acc_at(blk, e, lane)] = 0;
        }
    const i64 W = row[NB * 512];
    finalize<NB>(a, S, W, p, lane);                       // (every lane has read W before lane 0 clears it: the shuffles of the norm lie between)
    if (lane == 0) row[NB * 512] = 0;
}

template <int NB>
__global__ void __launch_bounds__(256) tpl_score(const TArgs a) {
    const int lane = threadIdx.x & 63;
    int p, m0, m1, nch, j;
    if (!chunk_of(a, blockIdx.x * 4 + (threadIdx.x >> 6), p, m0, m1, nch, j)) return;
    if (m0 >= m1) return;                                 // (a person without a member)
    const int pieces = a.dim >> 3;
    int32_t T[NB][8];
#pragma unroll
    for (int blk = 0; blk < NB; blk++) {
        const int piece = blk * 64 + lane;
        const u32x4 t = piece < pieces ? *(const u32x4 *)(a.tpl + (size_t)p * a.dim + piece * 8) : u32x4{0u, 0u, 0u, 0u};
        unpack8(t, T[blk]);
    }
    u64 low = ~0ull, high = 0ull;
    int keeps = 0, drops = 0;
    for (int b = m0; b < m1; b += 64) {
        const int idx = b + lane, cnt = min(64, m1 - b);
        const int myrow = idx < m1 ? a.lrow[idx] : 0;
        i64 mine = 0;
        for (int i0 = 0; i0 < cnt; i0 += 4) {
            u32x4 v[4][NB];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const bool live = i0 + u < cnt;
                const u32x4 *src = (const u32x4 *)(a.gal + (size_t)__shfl(myrow, (i0 + u) & 63) * a.dim * 2);
#pragma unroll
                for (int blk = 0; blk < NB; blk++) {
                    const int piece = blk * 64 + lane;
                    v[u][blk] = (live && piece < pieces) ? src[piece] : u32x4{0u, 0u, 0u, 0u};
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                i64 d = 0;
#pragma unroll
                for (int blk = 0; blk < NB; blk++) {
                    int32_t x[8];
                    unpack8(v[u][blk], x);
#pragma unroll
                    for (int e = 0; e < 8; e++) d += (i64)x[e] * (i64)T[blk][e];
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) d += (i64)shfl_xor_u64((u64)d, o);
                if (lane == i0 + u) mine = d;
            }
        }
        if (idx < m1) {
            const int pos = a.lpos[idx];
            const float s = fid_tpl_score(mine);
            const bool keep = a.keep_all || fid_tpl_keeps(s, a.min_score);
            a.score[pos] = s;
            a.kept[pos] = keep ? 1 : 0;
            a.lwk[idx] = keep ? a.lw[idx] : 0;
            const u64 kl = fid_tpl_low_key(__float_as_uint(s), pos), kh = fid_tpl_high_key(__float_as_uint(s), pos);
            low = kl < low ? kl : low;
            high = kh > high ? kh : high;
            keeps += keep;
            drops += !keep;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 l = shfl_xor_u64(low, o), h = shfl_xor_u64(high, o);
        low = l < low ? l : low;
        high = h > high ? h : high;
        keeps += __shfl_xor(keeps, o);
        drops += __shfl_xor(drops, o);
    }
    if (lane == 0) {
        atomicMin(a.klow + p, low);
        atomicMax(a.khigh + p, high);
        if (keeps) atomicAdd(a.keptc + p, keeps);
        if (drops) atomicAdd(a.summary + 3, (u64)drops);
    }
}

// a thread per person
__global__ void __launch_bounds__(256) tpl_report(const TArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool has = false, zero = false;
    if (p < a.P) {
        const int c = a.count[p];
        const u64 low = a.klow[p], high = a.khigh[p];
        has = c > 0;
        zero = !(a.cohesion[p] > 0.f);
        a.person[(size_t)p * 4 + 0] = c;
        a.person[(size_t)p * 4 + 1] = a.keptc[p];
        a.person[(size_t)p * 4 + 2] = has ? (int)(unsigned)low : -1;
        a.person[(size_t)p * 4 + 3] = has ? (int)~(unsigned)high : -1;
    }
    const int nh = __popcll(__ballot(has)), nz = __popcll(__ballot(zero));
    if (lane == 0 && nh) atomicAdd(a.summary + 1, (u64)nh);
    if (lane == 0 && nz) atomicAdd(a.summary + 2, (u64)nz);
}

// a wave per row: 16 bytes per lane and step, byte for byte
__global__ void __launch_bounds__(256) put_rows(const char *src, const int32_t *rows, int n, int dim, int G, char *gal) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int row = rows[i];
    if (row < 0 || row >= G) return;                      // (the call has checked them; a kernel never trusts an index it did not compute)
    const u32x4 *s = (const u32x4 *)(src + (size_t)i * dim * 2);
    u32x4 *d = (u32x4 *)(gal + (size_t)row * dim * 2);
    for (int k = lane; k < dim / 8; k += 64) d[k] = s[k];
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace fid

extern "C" {

int fid_gallery_templates(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const int32_t *labels_dev, const int32_t *weights_dev, int n, int P,
                          float min_score, void *templates_f16_dev, float *score_dev, int32_t *kept_dev, int32_t *person_dev, float *cohesion_dev,
                          int64_t *summary_dev) {
    using namespace fid;
    FID_REQUIRE(ctx && g && labels_dev && templates_f16_dev && score_dev && kept_dev && person_dev && cohesion_dev && summary_dev,
                "templates: NULL context, gallery, labels or output pointer");
    FID_REQUIRE(((uintptr_t)summary_dev & 7) == 0, "templates: summary_dev must be 8-byte aligned");
    FID_REQUIRE(((uintptr_t)templates_f16_dev & 15) == 0, "templates: templates_f16_dev must be 16-byte aligned");
    int G = 0, Gp = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, &Gp, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    if (!rows_dev) n = G;
    FID_REQUIRE(n > 0 && n <= FID_TEMPLATE_MAX_ROWS, "templates: %d rows (1 .. %d per call)", n, FID_TEMPLATE_MAX_ROWS);
    FID_REQUIRE(P > 0 && P <= n, "templates: %d persons (1 .. n = %d)", P, n);
    FID_REQUIRE(std::isfinite(min_score), "templates: min_score must be finite");
    FID_REQUIRE(dim > 0 && dim % 32 == 0 && dim <= FID_TEMPLATE_MAX_DIM, "templates: embedding dim %d must be a multiple of 32, at most %d", dim,
                FID_TEMPLATE_MAX_DIM);
    FID_REQUIRE((size_t)Gp * dim * 2 < 0xFFFFFF00ull, "templates: gallery larger than 4 GiB");
    // FID_TEMPLATE_CHUNK in the environment: the members one wave sums, read per call for measurements; the answer does not depend on it
    int chunk = FID_TEMPLATE_CHUNK;
    if (const char *e = getenv("FID_TEMPLATE_CHUNK")) chunk = atoi(e);
    FID_REQUIRE(chunk >= 16 && chunk <= 65536, "templates: FID_TEMPLATE_CHUNK=%d (16 .. 65536)", chunk);
    // FID_TEMPLATE_COMBINE=pass: split persons combine through partial rows and a second pass; anything else, or nothing: the int64 atomics
    const char *cmb = getenv("FID_TEMPLATE_COMBINE");
    const int combine = cmb && cmb[0] == 'p';
    const int nb = cdiv(dim, 512) <= 1 ? 1 : cdiv(dim, 512) <= 2 ? 2 : cdiv(dim, 512) <= 4 ? 4 : 8;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // scratch slot 2 (shared with fid_match / fid_gallery_group / fid_gallery_dedup / fid_gallery_cluster / fid_gallery_score_hist; calls are
    // serialised by the context's mutex and ordered by its stream), laid out for n rounded up to 65 536 so that the arena is replaced (behind a
    // stream synchronise, the rule of get_scratch) at most when a call crosses such a step
    const size_t ncap = ((size_t)n + 65535) & ~(size_t)65535;
    const size_t max_split = ncap / ((size_t)chunk + 1) + 1;
    const size_t acc_stride = (size_t)nb * 512 + 8;
    const size_t per_p = up256((ncap + 1) * 4), per_n = up256(ncap * 4);
    const size_t max_parts = combine ? 2 * ncap / (size_t)chunk + 1 : 0;
    const size_t zero_bytes = per_p;                                                  // count: what a call needs zeroed up front
    const size_t total = zero_bytes + max_split * acc_stride * 8 + max_parts * acc_stride * 8 + 6 * per_p + 2 * up256(ncap * 8) +
                         up256(max_split * 4) + up256(4 * SCAN * 4) + 256 + 4 * per_n;
    void *ws;
    FID_TRY(get_scratch(ctx, 2, total, &ws));
    TArgs a{};
    char *at = (char *)ws;
    auto take = [&](size_t bytes) { char *p = at; at += bytes; return p; };
    a.count = (int32_t *)take(per_p);
    a.acc = (i64 *)take(max_split * acc_stride * 8);
    a.part = (i64 *)take(max_parts * acc_stride * 8);
    a.pslot = (int32_t *)take(per_p);
    a.start = (int32_t *)take(per_p);
    a.cstart = (int32_t *)take(per_p);
    a.sslot = (int32_t *)take(per_p);
    a.cursor = (int32_t *)take(per_p);
    a.keptc = (int32_t *)take(per_p);
    a.klow = (u64 *)take(up256(ncap * 8));
    a.khigh = (u64 *)take(up256(ncap * 8));
    a.split_person = (int32_t *)take(up256(max_split * 4));
    a.bsum = (int32_t *)take(up256(4 * SCAN * 4));
    a.hdr = (int32_t *)take(256);
    a.lpos = (int32_t *)take(per_n);
    a.lrow = (int32_t *)take(per_n);
    a.lw = (int32_t *)take(per_n);
    a.lwk = (int32_t *)take(per_n);
    a.acc_stride = (int)acc_stride;
    a.gal = (const char *)rows; a.rows = rows_dev; a.labels = labels_dev; a.weights = weights_dev;
    a.n = n; a.P = P; a.G = G; a.dim = dim; a.chunk = chunk; a.combine = combine;
    a.min_score = min_score; a.keep_all = min_score <= -2.0f;
    a.tpl = (uint16_t *)templates_f16_dev; a.score = score_dev; a.kept = kept_dev; a.person = person_dev; a.cohesion = cohesion_dev;
    a.summary = (u64 *)summary_dev;
    FID_HIP(hipMemsetAsync(ws, 0, zero_bytes, ctx->stream));
    FID_HIP(hipMemsetAsync(summary_dev, 0, FID_TEMPLATE_SUMMARY_WORDS * 8, ctx->stream));
    const int scan_blocks = cdiv(P, SCAN);                // <= 1024: P <= 2^20
    const unsigned chunk_waves = (unsigned)P + (unsigned)(n / chunk) + 1u;             // every person one chunk, and one more per `chunk` members
    const dim3 cgrid((chunk_waves + 3) / 4), sgrid((unsigned)(((size_t)n / ((size_t)chunk + 1) + 1 + 3) / 4));
    hipLaunchKernelGGL(tpl_prepare, dim3(cdiv(cdiv(n, 64), 4)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(tpl_scan_a, dim3(scan_blocks), dim3(SCAN), 0, ctx->stream, a);
    hipLaunchKernelGGL(tpl_scan_b, dim3(1), dim3(SCAN), 0, ctx->stream, a, scan_blocks);
    hipLaunchKernelGGL(tpl_scan_c, dim3(scan_blocks), dim3(SCAN), 0, ctx->stream, a);
    if (!combine) hipLaunchKernelGGL(tpl_clear, sgrid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(tpl_scatter, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, a);
#define TPL_CHAIN(NB)                                                                                   \
    do {                                                                                                \
        hipLaunchKernelGGL((tpl_sum<NB, 0>), cgrid, dim3(256), 0, ctx->stream, a);                      \
        hipLaunchKernelGGL((tpl_finish<NB, 0>), sgrid, dim3(256), 0, ctx->stream, a);                   \
        hipLaunchKernelGGL(tpl_score<NB>, cgrid, dim3(256), 0, ctx->stream, a);                         \
        if (!a.keep_all) {                                                                              \
            hipLaunchKernelGGL((tpl_sum<NB, 1>), cgrid, dim3(256), 0, ctx->stream, a);                  \
            hipLaunchKernelGGL((tpl_finish<NB, 1>), sgrid, dim3(256), 0, ctx->stream, a);               \
        }                                                                                               \
    } while (0)
    switch (nb) { case 1: TPL_CHAIN(1); break; case 2: TPL_CHAIN(2); break; case 4: TPL_CHAIN(4); break; default: TPL_CHAIN(8); }
#undef TPL_CHAIN
    hipLaunchKernelGGL(tpl_report, dim3(cdiv(P, 256)), dim3(256), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_templates_host(const void *rows_f16, int G, int dim, const int32_t *rows, const int32_t *labels, const int32_t *weights, int n, int P,
                       float min_score, void *templates_f16, float *score, int32_t *kept, int32_t *person, float *cohesion, int64_t *summary) {
    if (!rows && rows_f16) n = G;
    const char *why = fid_templates_check(rows_f16, G, dim, labels, n, P, min_score, templates_f16, score, kept, person, cohesion, summary);
    FID_REQUIRE(why == nullptr, "templates host: %s", why ? why : "");
    fid_templates_table_host(rows_f16, G, dim, rows, labels, weights, n, P, min_score, templates_f16, score, kept, person, cohesion, summary);
    return FID_OK;
}

int fid_gallery_put_rows_f16(fid_ctx *ctx, fid_gallery *g, const int32_t *rows_dev, const void *src_f16_dev, int n) {
    using namespace fid;
    FID_REQUIRE(ctx && g && rows_dev && src_f16_dev, "put_rows_f16: NULL context, gallery, rows or source");
    FID_REQUIRE(n > 0 && n <= FID_TEMPLATE_MAX_ROWS, "put_rows_f16: %d rows (1 .. %d per call)", n, FID_TEMPLATE_MAX_ROWS);
    FID_REQUIRE(((uintptr_t)src_f16_dev & 15) == 0, "put_rows_f16: src_f16_dev must be 16-byte aligned");
    int G = 0, dim = 0;
    void *rows = nullptr;
    FID_TRY(fid_gallery_info(g, &G, nullptr, &dim));
    FID_TRY(fid_gallery_data(g, &rows));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    // the rows are checked on the host before anything is written: one small download behind the work enqueued so far
    std::vector<int32_t> host((size_t)n);
    FID_HIP(hipMemcpyAsync(host.data(), rows_dev, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) FID_REQUIRE(host[i] >= 0 && host[i] < G, "put_rows_f16: row %d outside the gallery (%d rows)", host[i], G);
    hipLaunchKernelGGL(put_rows, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, (const char *)src_f16_dev, rows_dev, n, dim, G, (char *)rows);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // extern "C"
