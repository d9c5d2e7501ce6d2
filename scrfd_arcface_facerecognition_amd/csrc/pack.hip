// Packed face lists: the per-frame face counts of the post-process as ONE dense row table across the batch, so that alignment,
// recogniser, normalisation and match run on (sum of faces) rows instead of B x (max faces per frame) slots.
// Serves reference main.py:130-134 (`detect(frame, max_num)` then one recogniser call per returned face) with
// models/scrfd.py:159-177 (max_num = 0 returns EVERY NMS survivor; only max_num > 0 selects).
//
//   k_b     = min(max(counts[b], 0), cap [, max_per_frame])
//   offsets = exclusive prefix sum of k_b, offsets[B] = total (NOT clipped to row_cap: overflow stays visible)
//   src[i]  = b * cap + f for the i-th face in (frame, rank) order, i < min(total, row_cap); -1 for the rows after them
//
// The consumers of the table (fid_align_crops_packed in align.hip, fid_l2_normalize_f16_packed in match.hip) live next to the
// code they share with the slot forms.
#include "common.h"

namespace {

constexpr int PACK_THREADS = 1024;       // 16 wavefronts: one chunk of the scan
constexpr int PACK_ROWS = 1024;          // rows of src one workgroup fills

// One launch, cdiv(row_cap, PACK_ROWS) workgroups.  EVERY workgroup scans all B counts itself (B / 1024 chunks of: one load, a 6-step
// wave64 shuffle scan, 16 wave totals through LDS) -- cheaper than a second launch or a grid-wide barrier -- and a frame's thread
// writes the part of the frame's faces that falls into its workgroup's row range.  Workgroup 0 also writes offsets.
__global__ void __launch_bounds__(PACK_THREADS) face_pack(const int *__restrict__ counts, int B, int cap, int max_per_frame,
                                                          int *__restrict__ offsets, int *__restrict__ src, int row_cap) {
    __shared__ int wave_sum[PACK_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = blockIdx.x * PACK_ROWS, hi = min(lo + PACK_ROWS, row_cap);
    int carry = 0;                       // faces of the frames before this chunk (<= B * cap, checked by the caller to fit an int)
    for (int b0 = 0; b0 < B; b0 += PACK_THREADS) {
        const int b = b0 + (int)threadIdx.x;
        int k = 0;
        if (b < B) {
            k = min(max(counts[b], 0), cap);
            if (max_per_frame > 0) k = min(k, max_per_frame);
        }
        int incl = k;                    // inclusive scan over the 64 lanes of the wavefront
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < PACK_THREADS / 64; w++) {
            const int s = wave_sum[w];
            before += w < wave ? s : 0;
            chunk += s;
        }
        const int off = carry + before + incl - k;
        if (b < B) {
            if (blockIdx.x == 0) offsets[b] = off;
            // faces [f0, f1) of this frame land in rows [lo, hi)
            const int f0 = max(lo - off, 0), f1 = min(k, hi - off);
            for (int f = f0; f < f1; f++) src[off + f] = b * cap + f;
        }
        carry += chunk;
        __syncthreads();                 // wave_sum is rewritten by the next chunk
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[B] = carry;
    for (int i = max(lo, carry) + (int)threadIdx.x; i < hi; i += PACK_THREADS) src[i] = -1;
}

}  // namespace

extern "C" {

int fid_face_pack(fid_ctx *ctx, const int32_t *counts_dev, int B, int cap, int max_per_frame, int32_t *offsets_dev, int32_t *src_dev,
                  int row_cap) {
    FID_REQUIRE(ctx && counts_dev && offsets_dev && src_dev, "NULL argument");
    FID_REQUIRE(B > 0 && cap > 0 && max_per_frame >= 0 && row_cap > 0, "bad sizes");
    FID_REQUIRE((long long)B * cap <= 0x7FFFFFFFll, "B * cap = %lld overflows the row table's int32 entries", (long long)B * cap);
    FID_REQUIRE(row_cap <= 0x7FFFFFFF - PACK_ROWS && B <= 0x7FFFFFFF - PACK_THREADS, "B %d / row_cap %d too large", B, row_cap);
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    hipLaunchKernelGGL(face_pack, dim3(fid::cdiv(row_cap, PACK_ROWS)), dim3(PACK_THREADS), 0, ctx->stream, counts_dev, B, cap, max_per_frame,
                       offsets_dev, src_dev, row_cap);
    FID_HIP(hipGetLastError());
    return FID_OK;
}

}  // extern "C"
