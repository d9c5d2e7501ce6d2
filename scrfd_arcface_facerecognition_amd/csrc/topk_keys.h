// The packed key of the top-k kernels and the merge that only sees keys, for topk_scan.hip (which defines the merge) and coarse.hip.
//   key = sortable(score) << 32 | ~(first_row + row): unsigned order = score descending, lowest row first; 0 = no candidate.
#pragma once
#include "common.h"

namespace fid {

typedef unsigned long long u64;

#ifdef __HIPCC__
__device__ __forceinline__ u64 make_key(float s, int row) {
    const unsigned u = __float_as_uint(s);
    return ((u64)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | (unsigned)~(unsigned)row;
}
__device__ __forceinline__ float key_score(u64 key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
// the list is sorted descending; `key` takes its place and the last entry falls out (every index static: the list stays in registers)
template <int KP>
__device__ __forceinline__ void list_insert(u64 (&l)[KP], u64 key) {
#pragma unroll
    for (int j = 0; j < KP; j++) {
        const u64 cur = l[j];
        const bool better = key > cur;
        l[j] = better ? key : cur;
        key = better ? cur : key;
    }
}
#endif

// the register list a kernel keeps for k results
inline int list_len(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// topk_merge (topk_scan.hip), one wave per query: the k largest of its parts x count keys, descending.  Keys that are 0 or name a row >= G_total
// are no candidates.  keys_out != NULL: the keys themselves ([n, k], 0 behind the last); otherwise (idx, score) under the strict threshold.
void launch_merge(fid_ctx *ctx, const u64 *keys, int parts, long long stride_p, long long stride_q, int count, int n, int k, int G_total,
                  float thresh, u64 *keys_out, int32_t *idx, float *score);

}  // namespace fid
