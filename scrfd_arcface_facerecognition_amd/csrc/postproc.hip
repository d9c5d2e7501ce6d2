// SCRFD post-process on the GPU: threshold + decode + compact, exact sort, greedy NMS, max_num.
// Replaces the numpy/python code of reference models/scrfd.py:89-178 (forward's decode loop and
// detect's sort / NMS / max_num) and :180-207 (nms), utils/helpers.py:62-107 (distance2bbox/kps).
//
// Bit-exactness contract: every fp32 operation below is a single correctly
// rounded IEEE operation in the same order numpy performs it (no FMA contraction: the explicit
// __f*_rn intrinsics forbid it), so given identical head tensors the survivors, their order and
// their coordinates are identical to the reference's.
//
// HBM-bound integer/fp32 work: one pass over the 16800 x 15 head values per frame (1.0 MB),
// everything after the threshold touches only the few candidates.
#include "common.h"

namespace {

constexpr int CAND_W = 16;  // floats per candidate record: x1 y1 x2 y2 score kps[10] orig_index

struct HeadViews {
    const float *ptr[9];
    int pix_stride[9];
    int anc_stride[9];
    long long batch_stride[9];
};
// the kernel argument from an entry point's four arrays of nine (the arrays themselves non-NULL: checked by the caller)
int head_views(const float *const head_dev[9], const int32_t pix_stride[9], const int32_t anc_stride[9], const int64_t batch_stride[9],
               HeadViews *hv) {
    for (int k = 0; k < 9; k++) {
        FID_REQUIRE(head_dev[k], "head %d is NULL", k);
        hv->ptr[k] = head_dev[k];
        hv->pix_stride[k] = pix_stride[k];
        hv->anc_stride[k] = anc_stride[k];
        hv->batch_stride[k] = batch_stride[k];
    }
    return FID_OK;
}

// (-0.0 takes +0.0's key: numpy's sort compares the two equal and leaves them in index order)
__device__ __forceinline__ unsigned sortable(float f) {
    unsigned u = __float_as_uint(f == 0.f ? 0.f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Where the candidates of head batch entry t go, and what scales them: the placement policy of decode_compact.
struct PlaceUniform {        // entry t is frame t; one det_scale for the batch.  by_index: anchor order instead of score order (fid_scrfd_decode)
    static constexpr bool tiled = false;
    float ds;
    int by_index;
    __device__ __forceinline__ float det_scale(int) const { return ds; }
};
struct PlaceRagged {         // a mixed-size batch: frame t's det_scale from the per-image table (block-uniform)
    static constexpr bool tiled = false;
    static constexpr int by_index = 0;
    const fid::RaggedImg *tab;
    __device__ __forceinline__ float det_scale(int t) const { return tab[t].det_scale; }
};
// Tiled detection: entry t is tile t of the table, its candidates join frame tab[t].frame's list in FRAME coordinates: every coordinate
// moves by the tile's origin, (v / det_scale) + (float)x0 or y0, two single rounded fp32 operations.  A candidate whose frame box comes
// within `margin` pixels of a side of the tile that is a cut (not the frame's boundary) is dropped before it takes a slot: the half face a
// tile sees at a cut (margin < 0: no rule).  Order inside a frame: score descending, then (tile rank, anchor) ascending -- what
// concatenating the tiles' candidate arrays in table order and the oracle's two stable sorts produce.
struct PlaceTiled {
    static constexpr bool tiled = true;
    static constexpr int by_index = 0;
    const fid::TileEntry *tab;
    int img_h, img_w, margin;
    __device__ __forceinline__ bool at_a_cut(const fid::TileEntry &e, const float (&xy)[4]) const {      // xy: the frame box x1 y1 x2 y2
        if (margin < 0) return false;
        return (e.x0 > 0 && xy[0] < (float)(e.x0 + margin)) || (e.y0 > 0 && xy[1] < (float)(e.y0 + margin)) ||
               (e.x0 + e.w < img_w && xy[2] > (float)(e.x0 + e.w - margin)) || (e.y0 + e.h < img_h && xy[3] > (float)(e.y0 + e.h - margin));
    }
};

// One thread per anchor.  scrfd.py:89-119 + :145-148 (the division by det_scale).  The untiled forms add no origin, not even 0.0f: that
// would turn a -0.0 into +0.0.
template <class Place>
__global__ void __launch_bounds__(256) decode_compact(HeadViews hv, int in_h, int in_w, int A, float thr, Place place, int cand_cap,
                                                      int *cand_count, unsigned long long *cand_key, float *cand_data) {
    const int n8 = (in_h / 8) * (in_w / 8) * A, n16 = (in_h / 16) * (in_w / 16) * A, n32 = (in_h / 32) * (in_w / 32) * A;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;  // flat anchor index over the 3 levels
    if (g >= n8 + n16 + n32) return;
    const int t = blockIdx.y;
    int lvl, i, stride;
    if (g < n8) { lvl = 0; i = g; stride = 8; }
    else if (g < n8 + n16) { lvl = 1; i = g - n8; stride = 16; }
    else { lvl = 2; i = g - n8 - n16; stride = 32; }
    const int pix = i / A, a = i - pix * A;
    const float score = hv.ptr[lvl][t * hv.batch_stride[lvl] + (long long)pix * hv.pix_stride[lvl] + a * hv.anc_stride[lvl]];
    if (!(score >= thr)) return;
    int b = t;
    unsigned idx = (unsigned)g;
    float ds, ox = 0.f, oy = 0.f;
    [[maybe_unused]] fid::TileEntry e;
    if constexpr (Place::tiled) {
        e = place.tab[t];
        b = e.frame; ds = e.det_scale; ox = (float)e.x0; oy = (float)e.y0;
        idx = (unsigned)e.rank * (unsigned)(n8 + n16 + n32) + (unsigned)g;   // < 2^31: checked by the launcher
    } else {
        ds = place.det_scale(t);
    }
    float *o = nullptr;                        // the candidate's record, once it has a slot
    unsigned long long *key = nullptr;
    auto take_slot = [&]() {
        const int slot = atomicAdd(&cand_count[b], 1);
        if (slot >= cand_cap) return false;    // overflow is reported through the count itself
        o = cand_data + ((size_t)b * cand_cap + slot) * CAND_W;
        key = cand_key + (size_t)b * cand_cap + slot;
        return true;
    };
    const int fw = in_w / stride;
    const float cx = (float)((pix % fw) * stride), cy = (float)((pix / fw) * stride);
    const float fs = (float)stride;
    const float *bp = hv.ptr[3 + lvl] + t * hv.batch_stride[3 + lvl] + (long long)pix * hv.pix_stride[3 + lvl] + a * hv.anc_stride[3 + lvl];
    // distance2bbox / distance2kps on (pred * stride), then / det_scale
    auto placed = [&](float v, float origin) { v = __fdiv_rn(v, ds); if constexpr (Place::tiled) v = __fadd_rn(v, origin); return v; };
    auto box = [&](float *d) {
        d[0] = placed(__fsub_rn(cx, __fmul_rn(bp[0], fs)), ox);
        d[1] = placed(__fsub_rn(cy, __fmul_rn(bp[1], fs)), oy);
        d[2] = placed(__fadd_rn(cx, __fmul_rn(bp[2], fs)), ox);
        d[3] = placed(__fadd_rn(cy, __fmul_rn(bp[3], fs)), oy);
    };
    if constexpr (Place::tiled) {              // box -> margin test -> slot
        float xy[4];
        box(xy);
        if (place.at_a_cut(e, xy)) return;
        if (!take_slot()) return;
        o[0] = xy[0]; o[1] = xy[1]; o[2] = xy[2]; o[3] = xy[3];
    } else {                                   // slot -> box, each value stored as it is decoded (27 VGPRs; four divisions in flight take 35)
        if (!take_slot()) return;
        box(o);
    }
    const float *kp = hv.ptr[6 + lvl] + t * hv.batch_stride[6 + lvl] + (long long)pix * hv.pix_stride[6 + lvl] + a * hv.anc_stride[6 + lvl];
    o[4] = score;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        o[5 + 2 * k] = placed(__fadd_rn(cx, __fmul_rn(kp[2 * k], fs)), ox);
        o[6 + 2 * k] = placed(__fadd_rn(cy, __fmul_rn(kp[2 * k + 1], fs)), oy);
    }
    o[15] = __int_as_float((int)idx);
    // order: score descending, then flat anchor index ascending (what a stable argsort()[::-1]
    // followed by nms()'s own stable argsort()[::-1] produces; identical to any order when tie-free)
    *key = place.by_index ? ((unsigned long long)(~idx) << 32) : (((unsigned long long)sortable(score) << 32) | (unsigned)(~idx));
}

// distance2bbox / distance2kps on plain arrays (utils/helpers.py:62-107): ncol = 4 -> bbox, else kps pairs
__global__ void decode_points(const float *points, const float *dist, int n, int ncol, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ncol) return;
    const int r = i / ncol, c = i - r * ncol;
    const float p = points[r * 2 + (c & 1)];
    out[i] = (ncol == 4 && c < 2) ? __fsub_rn(p, dist[i]) : __fadd_rn(p, dist[i]);
}

// fid_nms entry: records from a plain [K,5] det array.  Order: score desc, index DESC
// (scores.argsort()[::-1] with a stable sort, scrfd.py:188).
__global__ void load_dets(const float *dets, int K, int *cand_count, unsigned long long *cand_key, float *cand_data) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) cand_count[0] = K;
    if (i >= K) return;
    float *o = cand_data + (size_t)i * CAND_W;
    for (int k = 0; k < 5; k++) o[k] = dets[i * 5 + k];
    for (int k = 5; k < 15; k++) o[k] = 0.f;
    o[15] = __int_as_float(i);
    cand_key[i] = ((unsigned long long)sortable(dets[i * 5 + 4]) << 32) | (unsigned)i;
}

// Exact sort by counting: rank = number of keys that come before mine (keys are unique).
// O(K^2) per frame but K is tens..hundreds after the 0.5 threshold; no capacity or pow2 limits.
__global__ void __launch_bounds__(256) rank_scatter(const int *cand_count, const unsigned long long *cand_key,
                                                    const float *cand_data, float *sorted, int cand_cap) {
    const int b = blockIdx.y;
    const int K = min(cand_count[b], cand_cap);
    if ((int)(blockIdx.x * 256) >= K) return;
    __shared__ unsigned long long tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long *keys = cand_key + (size_t)b * cand_cap;
    const unsigned long long mine = i < K ? keys[i] : 0ull;
    int rank = 0;
    for (int t0 = 0; t0 < K; t0 += 256) {
        __syncthreads();
        tile[threadIdx.x] = (t0 + (int)threadIdx.x < K) ? keys[t0 + threadIdx.x] : 0ull;
        __syncthreads();
        const int n = min(256, K - t0);
        for (int j = 0; j < n; j++) rank += tile[j] > mine;
    }
    if (i < K) {
        const float4 *src = (const float4 *)(cand_data + ((size_t)b * cand_cap + i) * CAND_W);
        float4 *dst = (float4 *)(sorted + ((size_t)b * cand_cap + rank) * CAND_W);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    }
}

constexpr int NMS_MASK_K = 512;   // candidate lists up to this length take the bit-mask path of nms_select (32 KB of masks)

// Greedy NMS (scrfd.py:187-205) + max_num selection (scrfd.py:159-177).  One workgroup per frame.
// LDS: removed[cand_cap] bytes | keep[cand_cap] ints | value[cand_cap] floats | box[n_box] float4 | sup[NMS_MASK_K][NMS_MASK_K/32] masks.
// The boxes of the n_box best candidates are staged in LDS: the greedy loop is one iteration + barrier per surviving candidate, and
// reading candidate i's box from global memory put a trip to L2 (~0.3 us) on every iteration (29 us per 64-frame step).
// The body is shared by the uniform kernel and the mixed-size one, which differ only in where frame b's img_h, img_w come from.
__device__ __forceinline__ void nms_select_frame(unsigned char *smem, int b, const int *cand_count, const float *sorted, int cand_cap,
                                                 float iou_thr, int max_num, int metric, int img_h, int img_w, float *det_out,
                                                 float *kps_out, int *counts_out, int out_cap, int *keep_idx_out,
                                                 int *status, int n_box, int mask_ok) {
    const int Kraw = cand_count[b];
    const int K = min(Kraw, cand_cap);
    unsigned char *removed = smem;
    int *keep = (int *)(smem + ((cand_cap + 15) & ~15));
    float *value = (float *)(keep + cand_cap);
    const float *rec = sorted + (size_t)b * cand_cap * CAND_W;
    float4 *box = (float4 *)(smem + ((((cand_cap + 15) & ~15) + (size_t)cand_cap * 8 + 15) & ~(size_t)15));
    const int KB = min(K, n_box);
    for (int j = threadIdx.x; j < K; j += blockDim.x) removed[j] = 0;
    for (int j = threadIdx.x; j < KB; j += blockDim.x) box[j] = *(const float4 *)(rec + j * CAND_W);
    __syncthreads();
    int nkeep = 0;
    if (mask_ok && K <= NMS_MASK_K && K <= n_box) {
        // Small candidate lists (the usual case: tens to a few hundred per frame): all pairwise decisions first, in parallel, as bit
        // masks -- sup[i] bit j = "i suppresses j" = !(ovr(i, j) <= thr), j > i -- then ONE wave walks the list in score order and ORs
        // the masks of the candidates it keeps.  Same arithmetic, same decisions as the loop below (every operation of the overlap is
        // commutative in (i, j)); the loop's barrier per surviving candidate (8 waves, ~0.25 us each) is gone.
        constexpr int MW = NMS_MASK_K / 64;                      // 64-bit words per row
        unsigned long long *sup = (unsigned long long *)(box + n_box);   // [K][MW]
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, nwv = blockDim.x >> 6;
        const int KW = (K + 63) >> 6;                            // words in use
        for (int i = wv; i < K; i += nwv) {                      // a wave per row i, a lane per column j, one ballot per 64 columns
            const float4 bi = box[i];
            const float area_i = __fmul_rn(__fadd_rn(__fsub_rn(bi.z, bi.x), 1.f), __fadd_rn(__fsub_rn(bi.w, bi.y), 1.f));
            for (int w = 0; w < KW; w++) {
                const int j = w * 64 + ln;
                bool hit = false;
                if (w * 64 + 63 > i && j > i && j < K) {
                    const float4 bj = box[j];
                    const float area_j = __fmul_rn(__fadd_rn(__fsub_rn(bj.z, bj.x), 1.f), __fadd_rn(__fsub_rn(bj.w, bj.y), 1.f));
                    const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y), xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
                    const float w_ = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f));
                    const float h_ = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
                    const float inter = __fmul_rn(w_, h_);
                    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_i, area_j), inter));
                    hit = !(ovr <= iou_thr);
                }
                const unsigned long long m = __ballot(hit);
                if (ln == 0) sup[i * MW + w] = m;
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                  // one wave: lane l owns word l of the removed mask (MW <= 64)
            const int l = threadIdx.x;
            constexpr int MW2 = NMS_MASK_K / 64;
            const unsigned long long *sup2 = (const unsigned long long *)(box + n_box);
            unsigned long long gone = 0;
            for (int i = 0; i < K; i++) {
                const unsigned long long wi = __shfl(gone, i >> 6);   // (uniform across the wave)
                if ((wi >> (i & 63)) & 1ull) continue;
                if (l == 0) keep[nkeep] = i;
                nkeep++;
                if (l < MW2) gone |= sup2[i * MW2 + l];
            }
            if (l == 0) value[0] = __int_as_float(nkeep);        // hand the count to the other waves
        }
        __syncthreads();
        nkeep = __float_as_int(value[0]);
        __syncthreads();
    } else
    for (int i = 0; i < K; i++) {
        if (removed[i]) continue;  // uniform: written only before the previous barrier
        if (threadIdx.x == 0) keep[nkeep] = i;
        nkeep++;
        const float4 bi = i < KB ? box[i] : *(const float4 *)(rec + i * CAND_W);
        const float x1 = bi.x, y1 = bi.y, x2 = bi.z, y2 = bi.w;
        const float area_i = __fmul_rn(__fadd_rn(__fsub_rn(x2, x1), 1.f), __fadd_rn(__fsub_rn(y2, y1), 1.f));
        for (int j = i + 1 + threadIdx.x; j < K; j += blockDim.x) {
            if (removed[j]) continue;
            const float4 bj = j < KB ? box[j] : *(const float4 *)(rec + j * CAND_W);
            const float area_j = __fmul_rn(__fadd_rn(__fsub_rn(bj.z, bj.x), 1.f), __fadd_rn(__fsub_rn(bj.w, bj.y), 1.f));
            const float xx1 = fmaxf(x1, bj.x), yy1 = fmaxf(y1, bj.y), xx2 = fminf(x2, bj.z), yy2 = fminf(y2, bj.w);
            const float w = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f));
            const float h = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
            const float inter = __fmul_rn(w, h);
            const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_i, area_j), inter));
            if (!(ovr <= iou_thr)) removed[j] = 1;  // np.where(ovr <= thr) keeps; NaN is dropped
        }
        __syncthreads();
    }
    __syncthreads();
    // ---- selection / output ----
    const bool select = (max_num > 0) && (max_num < nkeep);
    if (select) {
        const float cxi = (float)(img_w / 2), cyi = (float)(img_h / 2);  // image_center = (H//2, W//2)
        for (int k = threadIdx.x; k < nkeep; k += blockDim.x) {
            const float *r = rec + keep[k] * CAND_W;
            const float area = __fmul_rn(__fsub_rn(r[2], r[0]), __fsub_rn(r[3], r[1]));
            float v = area;
            if (metric != 0) {
                const float ox = __fsub_rn(__fdiv_rn(__fadd_rn(r[0], r[2]), 2.f), cxi);
                const float oy = __fsub_rn(__fdiv_rn(__fadd_rn(r[1], r[3]), 2.f), cyi);
                const float d2 = __fadd_rn(__fmul_rn(ox, ox), __fmul_rn(oy, oy));
                v = __fsub_rn(area, __fmul_rn(d2, 2.f));
            }
            value[k] = v;
        }
        __syncthreads();
    }
    const int n_out = select ? max_num : nkeep;
    for (int k = threadIdx.x; k < nkeep; k += blockDim.x) {
        int p = k;
        if (select) {  // np.argsort(values)[::-1][:max_num], stable: larger value first, ties -> larger index first
            // numpy sorts NaN behind every number, so reversed it comes FIRST (inf - inf of a box with an infinite side), NaNs tie with each other
            const float v = value[k];
            const bool vnan = v != v;
            int rank = 0;
            for (int j = 0; j < nkeep; j++) {
                const float u = value[j];
                const bool unan = u != u;
                rank += vnan ? (unan && j > k) : (unan || u > v || (u == v && j > k));
            }
            p = rank < max_num ? rank : -1;
        }
        if (p < 0 || p >= out_cap) continue;
        const float *r = rec + keep[k] * CAND_W;
        if (det_out) {
            float *d = det_out + ((size_t)b * out_cap + p) * 5;
            for (int c = 0; c < 5; c++) d[c] = r[c];
        }
        if (kps_out) {
            float *q = kps_out + ((size_t)b * out_cap + p) * 10;
            for (int c = 0; c < 10; c++) q[c] = r[5 + c];
        }
        if (keep_idx_out) keep_idx_out[(size_t)b * out_cap + p] = __float_as_int(r[15]);
    }
    if (threadIdx.x == 0) {
        counts_out[b] = min(n_out, out_cap);
        atomicMax(&status[0], Kraw);
        atomicMax(&status[1], n_out);
    }
}

__global__ void __launch_bounds__(512) nms_select(const int *cand_count, const float *sorted, int cand_cap, float iou_thr,
                                                  int max_num, int metric, int img_h, int img_w, float *det_out,
                                                  float *kps_out, int *counts_out, int out_cap, int *keep_idx_out,
                                                  int *status, int n_box, int mask_ok) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    nms_select_frame(smem, blockIdx.x, cand_count, sorted, cand_cap, iou_thr, max_num, metric, img_h, img_w, det_out, kps_out, counts_out,
                     out_cap, keep_idx_out, status, n_box, mask_ok);
}

// a mixed-size batch: frame b's image size (the centre of the max_num metric, scrfd.py:169-172) from the per-image table
__global__ void __launch_bounds__(512) nms_select_ragged(const int *cand_count, const float *sorted, int cand_cap, float iou_thr,
                                                         int max_num, int metric, const fid::RaggedImg *tab, float *det_out,
                                                         float *kps_out, int *counts_out, int out_cap, int *status, int n_box, int mask_ok) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const fid::RaggedImg g = tab[blockIdx.x];
    nms_select_frame(smem, blockIdx.x, cand_count, sorted, cand_cap, iou_thr, max_num, metric, g.H, g.W, det_out, kps_out, counts_out,
                     out_cap, (int *)nullptr, status, n_box, mask_ok);
}

}  // namespace

namespace fid {
// dynamic LDS of nms_select for a candidate capacity, and how many boxes fit behind the per-candidate arrays (at most 1024)
static size_t nms_lds_bytes(int cand_cap, int *n_box) {
    const size_t base = ((((size_t)cand_cap + 15) & ~(size_t)15) + (size_t)cand_cap * 8 + 15) & ~(size_t)15;
    const size_t masks = (size_t)NMS_MASK_K * (NMS_MASK_K / 64) * 8;          // 32 KB, only when they fit beside >= NMS_MASK_K boxes
    const size_t room = base < 160 * 1024 ? (160 * 1024 - base) / 16 : 0;
    int nb = (int)std::min<size_t>(1024, room);
    const bool with_masks = base + (size_t)NMS_MASK_K * 16 + masks <= 160 * 1024;
    if (with_masks) nb = (int)std::min<size_t>(1024, (160 * 1024 - base - masks) / 16);
    else nb = std::min(nb, NMS_MASK_K - 1);                                    // fewer boxes than NMS_MASK_K: the kernel never takes the mask path
    if (n_box) *n_box = with_masks ? nb : -nb;                                 // (negative: no mask area behind the boxes)
    return base + (size_t)nb * 16 + (with_masks ? masks : 0);
}
// FID_KLOG=1: the two values that pick nms_select's path, as handed to the launch (tests/nms_cases.py mirrors them; n_box as nms_lds_bytes returns it)
static void klog_nms(int cand_cap, int n_box) {
    static const bool klog = getenv("FID_KLOG") != nullptr;
    if (klog) fprintf(stderr, "[klog] nms cand_cap %d n_box %d masks %d\n", cand_cap, n_box < 0 ? -n_box : n_box, n_box > 0 ? 1 : 0);
}
// shared by fid_scrfd_postprocess and the fused pipeline
// tab != NULL: a mixed-size batch -- det_scale and the image size of frame b come from tab[b], img_h / img_w are unused
// tiles != NULL: tiled detection -- the heads hold T tiles, whose candidates join the lists of the B frames they were cut from (PlaceTiled)
int scrfd_postprocess_launch(fid_ctx *ctx, const HeadViews &hv, int B, int in_h, int in_w, int A, int img_h, int img_w,
                             float conf, float iou, int max_num, int metric, float *det_dev, float *kps_dev,
                             int32_t *counts_dev, int cap, const RaggedImg *tab = nullptr, const TileEntry *tiles = nullptr, int T = 0,
                             int edge_margin = -1) {
    const int cc = ctx->cand_cap;
    // workspace: counts | keys | records | sorted records
    const size_t off_keys = ((size_t)B * 4 + 255) & ~(size_t)255;
    const size_t off_data = off_keys + (size_t)B * cc * 8;
    const size_t off_sorted = off_data + (size_t)B * cc * CAND_W * 4;
    const size_t total = off_sorted + (size_t)B * cc * CAND_W * 4;
    void *ws;
    FID_TRY(get_scratch(ctx, 0, total, &ws));
    int *cand_count = (int *)ws;
    auto *keys = (unsigned long long *)((char *)ws + off_keys);
    float *data = (float *)((char *)ws + off_data);
    float *sorted = (float *)((char *)ws + off_sorted);
    // (a degenerate letterbox is not refused here: its det_scale, 0.0f when new_h is 0, divides like the reference's)
    RaggedImg geom{};
    ragged_geometry(img_h, img_w, in_h, in_w, &geom);
    FID_HIP(hipMemsetAsync(cand_count, 0, (size_t)B * 4, ctx->stream));
    const int total_anchors = ((in_h / 8) * (in_w / 8) + (in_h / 16) * (in_w / 16) + (in_h / 32) * (in_w / 32)) * A;
    auto decode = [&](auto place, int n) {       // n head batch entries
        hipLaunchKernelGGL(decode_compact<decltype(place)>, dim3(cdiv(total_anchors, 256), n), dim3(256), 0, ctx->stream, hv, in_h, in_w, A, conf,
                           place, cc, cand_count, keys, data);
    };
    if (tiles) decode(PlaceTiled{tiles, img_h, img_w, edge_margin}, T);
    else if (tab) decode(PlaceRagged{tab}, B);
    else decode(PlaceUniform{geom.det_scale, 0}, B);
    dim3 g2(cdiv(cc, 256), B);
    hipLaunchKernelGGL(rank_scatter, g2, dim3(256), 0, ctx->stream, cand_count, keys, data, sorted, cc);
    int n_box = 0;
    const size_t lds = nms_lds_bytes(cc, &n_box);
    klog_nms(cc, n_box);
    if (tab)
        hipLaunchKernelGGL(nms_select_ragged, dim3(B), dim3(512), lds, ctx->stream, cand_count, sorted, cc, iou, max_num, metric, tab,
                           det_dev, kps_dev, counts_dev, cap, ctx->status_dev, n_box < 0 ? -n_box : n_box, n_box > 0);
    else
        hipLaunchKernelGGL(nms_select, dim3(B), dim3(512), lds, ctx->stream, cand_count, sorted, cc, iou, max_num, metric, img_h,
                           img_w, det_dev, kps_dev, counts_dev, cap, (int *)nullptr, ctx->status_dev, n_box < 0 ? -n_box : n_box, n_box > 0);
    FID_HIP(hipGetLastError());
    ctx->last_out_cap = cap;
    return FID_OK;
}
}  // namespace fid

extern "C" {

int fid_scrfd_set_candidate_capacity(fid_ctx *ctx, int cand_cap) {
    FID_REQUIRE(ctx, "ctx is NULL");
    // LDS of nms_select: ~9 bytes per candidate; 16800 anchors -> 151 KB of the CU's 160 KB
    FID_REQUIRE(cand_cap >= 16 && cand_cap <= 16800, "cand_cap %d outside [16, 16800]", cand_cap);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    ctx->cand_cap = cand_cap;
    FID_TRY(fid::ensure_dyn_lds(ctx, (const void *)nms_select, (int)fid::nms_lds_bytes(cand_cap, nullptr)));
    return FID_OK;
}

int fid_scrfd_postprocess(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                          const int32_t anc_stride[9], const int64_t batch_stride[9], int B, int in_h, int in_w,
                          int num_anchors, int img_h, int img_w, float conf_thres, float iou_thres, int max_num,
                          int metric, float *det_dev, float *kps_dev, int32_t *counts_dev, int cap) {
    FID_REQUIRE(ctx && head_dev && pix_stride && anc_stride && batch_stride, "NULL argument");
    FID_REQUIRE(B > 0 && cap > 0 && det_dev && kps_dev && counts_dev, "bad batch/capacity/output");
    FID_REQUIRE(in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0, "input size %dx%d not a multiple of 32", in_w, in_h);
    FID_REQUIRE(img_h > 0 && img_w > 0 && num_anchors > 0, "bad image size / anchors");
    FID_REQUIRE(metric == 0 || metric == 1, "metric must be 0 (max) or 1 (default)");
    HeadViews hv;
    FID_TRY(head_views(head_dev, pix_stride, anc_stride, batch_stride, &hv));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_TRY(fid::ensure_dyn_lds(ctx, (const void *)nms_select, (int)fid::nms_lds_bytes(ctx->cand_cap, nullptr)));   // (above 64 KB from ~2000 candidates on)
    return fid::scrfd_postprocess_launch(ctx, hv, B, in_h, in_w, num_anchors, img_h, img_w, conf_thres, iou_thres, max_num,
                                         metric, det_dev, kps_dev, counts_dev, cap);
}

// A mixed-size batch (the reference runs scrfd.py:145-148,159-177 per image): frame b came from an H_b x W_b image, hw = host [B,2].
int fid_scrfd_postprocess_ragged(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                                 const int32_t anc_stride[9], const int64_t batch_stride[9], int B, int in_h, int in_w,
                                 int num_anchors, const int32_t *hw, float conf_thres, float iou_thres, int max_num,
                                 int metric, float *det_dev, float *kps_dev, int32_t *counts_dev, int cap) {
    FID_REQUIRE(ctx && head_dev && pix_stride && anc_stride && batch_stride && hw, "NULL argument");
    FID_REQUIRE(B > 0 && cap > 0 && det_dev && kps_dev && counts_dev, "bad batch/capacity/output");
    FID_REQUIRE(in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0, "input size %dx%d not a multiple of 32", in_w, in_h);
    FID_REQUIRE(num_anchors > 0, "bad anchors");
    FID_REQUIRE(metric == 0 || metric == 1, "metric must be 0 (max) or 1 (default)");
    HeadViews hv;
    FID_TRY(head_views(head_dev, pix_stride, anc_stride, batch_stride, &hv));
    std::vector<fid::RaggedImg> host(B);
    for (int b = 0; b < B; b++) {
        FID_REQUIRE(hw[2 * b] > 0 && hw[2 * b + 1] > 0, "image %d: bad size %dx%d", b, hw[2 * b + 1], hw[2 * b]);
        FID_REQUIRE(fid::ragged_geometry(hw[2 * b], hw[2 * b + 1], in_h, in_w, &host[b]), "image %d: degenerate letterbox %dx%d", b,
                    host[b].new_w, host[b].new_h);
        host[b].off = 0;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_TRY(fid::ensure_dyn_lds(ctx, (const void *)nms_select_ragged, (int)fid::nms_lds_bytes(ctx->cand_cap, nullptr)));
    const fid::RaggedImg *tab;
    FID_TRY(fid::ragged_table(ctx, host.data(), B, &tab));
    return fid::scrfd_postprocess_launch(ctx, hv, B, in_h, in_w, num_anchors, 1, 1, conf_thres, iou_thres, max_num, metric, det_dev,
                                         kps_dev, counts_dev, cap, tab);
}

// Tiled detection: the heads of T tiles (fid_tile_cut's output through the detector) merged per frame.  tiles: host [T,6], the table
// fid_tile_cut took; B frames of img_h x img_w.  Sort, NMS, max_num and the capacity report are those of fid_scrfd_postprocess, over B frames.
int fid_scrfd_postprocess_tiled(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9],
                                const int32_t anc_stride[9], const int64_t batch_stride[9], const int32_t *tiles, int T,
                                int in_h, int in_w, int num_anchors, int B, int img_h, int img_w, float conf_thres, float iou_thres,
                                int edge_margin, int max_num, int metric, float *det_dev, float *kps_dev, int32_t *counts_dev, int cap) {
    FID_REQUIRE(ctx && head_dev && pix_stride && anc_stride && batch_stride && tiles, "NULL argument");
    FID_REQUIRE(B > 0 && T > 0 && T <= 65535 && cap > 0 && det_dev && kps_dev && counts_dev, "bad batch/tiles/capacity/output");
    FID_REQUIRE(in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0, "input size %dx%d not a multiple of 32", in_w, in_h);
    FID_REQUIRE(img_h > 0 && img_w > 0 && num_anchors > 0, "bad image size / anchors");
    FID_REQUIRE(metric == 0 || metric == 1, "metric must be 0 (max) or 1 (default)");
    HeadViews hv;
    FID_TRY(head_views(head_dev, pix_stride, anc_stride, batch_stride, &hv));
    std::vector<fid::TileEntry> host;
    int per_frame = 0;
    FID_TRY(fid::tile_entries(tiles, T, B, img_h, img_w, in_h, in_w, host, &per_frame));
    const long long total_anchors = ((long long)(in_h / 8) * (in_w / 8) + (long long)(in_h / 16) * (in_w / 16) + (long long)(in_h / 32) * (in_w / 32)) * num_anchors;
    FID_REQUIRE(per_frame * total_anchors < (1ll << 31), "%d tiles of %lld anchors in one frame overflow the sort key's index", per_frame, total_anchors);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    FID_TRY(fid::ensure_dyn_lds(ctx, (const void *)nms_select, (int)fid::nms_lds_bytes(ctx->cand_cap, nullptr)));
    const fid::TileEntry *tab;
    FID_TRY(fid::tile_table(ctx, host.data(), T, &tab));
    return fid::scrfd_postprocess_launch(ctx, hv, B, in_h, in_w, num_anchors, img_h, img_w, conf_thres, iou_thres, max_num, metric, det_dev,
                                         kps_dev, counts_dev, cap, nullptr, tab, T, edge_margin);
}

// SCRFD.forward's decode loop alone (scrfd.py:89-119): candidates >= threshold in anchor order
// (levels 8,16,32 concatenated), NOT divided by det_scale.  rec_dev: [B, cand_cap, 16] floats
// (x1 y1 x2 y2 score kps[10] flat_anchor_index-as-int), counts_dev [B].
int fid_scrfd_decode(fid_ctx *ctx, const float *const head_dev[9], const int32_t pix_stride[9], const int32_t anc_stride[9],
                     const int64_t batch_stride[9], int B, int in_h, int in_w, int num_anchors, float conf_thres,
                     float *rec_dev, int32_t *counts_dev) {
    FID_REQUIRE(ctx && head_dev && pix_stride && anc_stride && batch_stride && rec_dev && counts_dev, "NULL argument");
    FID_REQUIRE(B > 0 && in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0 && num_anchors > 0, "bad sizes");
    HeadViews hv;
    FID_TRY(head_views(head_dev, pix_stride, anc_stride, batch_stride, &hv));
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    const int cc = ctx->cand_cap;
    const size_t off_keys = ((size_t)B * 4 + 255) & ~(size_t)255, off_data = off_keys + (size_t)B * cc * 8;
    void *ws;
    FID_TRY(fid::get_scratch(ctx, 0, off_data + (size_t)B * cc * CAND_W * 4, &ws));
    int *cand_count = (int *)ws;
    auto *keys = (unsigned long long *)((char *)ws + off_keys);
    float *data = (float *)((char *)ws + off_data);
    FID_HIP(hipMemsetAsync(cand_count, 0, (size_t)B * 4, ctx->stream));
    const int total = ((in_h / 8) * (in_w / 8) + (in_h / 16) * (in_w / 16) + (in_h / 32) * (in_w / 32)) * num_anchors;
    hipLaunchKernelGGL(decode_compact<PlaceUniform>, dim3(fid::cdiv(total, 256), B), dim3(256), 0, ctx->stream, hv, in_h, in_w, num_anchors,
                       conf_thres, PlaceUniform{1.0f, 1}, cc, cand_count, keys, data);
    hipLaunchKernelGGL(rank_scatter, dim3(fid::cdiv(cc, 256), B), dim3(256), 0, ctx->stream, cand_count, keys, data, rec_dev, cc);
    FID_HIP(hipMemcpyAsync(counts_dev, cand_count, (size_t)B * 4, hipMemcpyDeviceToDevice, ctx->stream));
    FID_HIP(hipGetLastError());
    return FID_OK;
}

// utils/helpers.py:62-83 / :86-107 on device arrays: points [n,2], distance [n,ncol] -> out [n,ncol]
int fid_distance2bbox(fid_ctx *ctx, const float *points_dev, const float *dist_dev, int n, float *out_dev) {
    FID_REQUIRE(ctx && points_dev && dist_dev && out_dev && n > 0, "bad args");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    hipLaunchKernelGGL(decode_points, dim3(fid::cdiv(n * 4, 256)), dim3(256), 0, ctx->stream, points_dev, dist_dev, n, 4, out_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}
int fid_distance2kps(fid_ctx *ctx, const float *points_dev, const float *dist_dev, int n, int ncol, float *out_dev) {
    FID_REQUIRE(ctx && points_dev && dist_dev && out_dev && n > 0 && ncol > 0 && ncol % 2 == 0 && ncol != 4, "bad args");
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    hipLaunchKernelGGL(decode_points, dim3(fid::cdiv(n * ncol, 256)), dim3(256), 0, ctx->stream, points_dev, dist_dev, n, ncol, out_dev);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

int fid_scrfd_check(fid_ctx *ctx, int *max_candidates) {
    FID_REQUIRE(ctx, "ctx is NULL");
    int st[2] = {0, 0};
    FID_HIP(hipMemcpyAsync(st, ctx->status_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    FID_HIP(hipStreamSynchronize(ctx->stream));
    FID_HIP(hipMemsetAsync(ctx->status_dev, 0, 8, ctx->stream));
    if (max_candidates) *max_candidates = st[0];
    if (st[0] > ctx->cand_cap) {
        fid::set_error("a frame produced %d candidates >= conf_thres but the workspace holds %d "
                       "(fid_scrfd_set_candidate_capacity)", st[0], ctx->cand_cap);
        return FID_E_CAPACITY;
    }
    if (st[1] > ctx->last_out_cap) {
        fid::set_error("a frame kept %d detections but the output capacity is %d", st[1], ctx->last_out_cap);
        return FID_E_CAPACITY;
    }
    return FID_OK;
}

// SCRFD.nms(dets, iou_thres) (scrfd.py:180-207) on a plain [K,5] array: keep indices into dets.
int fid_nms(fid_ctx *ctx, const float *dets_dev, int K, float iou_thres, int32_t *keep_dev, int32_t *count_dev) {
    FID_REQUIRE(ctx && keep_dev && count_dev && K >= 0, "bad args");
    FID_REQUIRE(K <= 16800, "K=%d exceeds 16800", K);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    if (K == 0) { FID_HIP(hipMemsetAsync(count_dev, 0, 4, ctx->stream)); return FID_OK; }
    FID_REQUIRE(dets_dev, "dets is NULL");
    const int cc = K;
    const size_t off_keys = 256, off_data = off_keys + (size_t)cc * 8, off_sorted = off_data + (size_t)cc * CAND_W * 4;
    void *ws;
    FID_TRY(fid::get_scratch(ctx, 0, off_sorted + (size_t)cc * CAND_W * 4, &ws));
    int *cand_count = (int *)ws;
    auto *keys = (unsigned long long *)((char *)ws + off_keys);
    float *data = (float *)((char *)ws + off_data);
    float *sorted = (float *)((char *)ws + off_sorted);
    hipLaunchKernelGGL(load_dets, dim3(fid::cdiv(K, 256)), dim3(256), 0, ctx->stream, dets_dev, K, cand_count, keys, data);
    hipLaunchKernelGGL(rank_scatter, dim3(fid::cdiv(cc, 256), 1), dim3(256), 0, ctx->stream, cand_count, keys, data, sorted, cc);
    int n_box = 0;
    const size_t lds = fid::nms_lds_bytes(cc, &n_box);
    fid::klog_nms(cc, n_box);
    FID_TRY(fid::ensure_dyn_lds(ctx, (const void *)nms_select, (int)std::max<size_t>(lds, fid::nms_lds_bytes(ctx->cand_cap, nullptr))));
    hipLaunchKernelGGL(nms_select, dim3(1), dim3(512), lds, ctx->stream, cand_count, sorted, cc, iou_thres, 0, 0, 1, 1,
                       (float *)nullptr, (float *)nullptr, count_dev, K, keep_dev, ctx->status_dev + 4, n_box < 0 ? -n_box : n_box, n_box > 0);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // extern "C"
