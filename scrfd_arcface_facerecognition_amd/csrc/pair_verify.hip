// Batch 1:1 verification: P pairs of embeddings -> P (score, verdict) records plus the counters of the reference's batch loop.
//
// reference smart_face_recognition.py:878-963 (compare_face_images: the two error returns :896-903 / :915-922, then faces[0] of each image,
// `similarity > self.similarity_thresh`, :928-932), :965-982 (calculate_face_similarity: np.dot(a, b) / (norm(a) * norm(b)) on the raw fp32
// embeddings) and the tallies of process_face_comparisons (:1088-1094, :1108-1110).
//
// The embeddings are read where the recogniser wrote them: raw fp32 rows, no normalised copy, no fp16.  One 64-lane wave per pair, four pairs
// per workgroup.  Lane l reads float4 l, l + 64, ... of both rows (1 KiB per wave-load) and keeps three fp32 partial sums -- a.b, a.a, b.b --
// which a xor-butterfly of wave shuffles reduces in a fixed order: the score is bitwise the same from run to run.  They are combined in the
// reference's order, dot / (sqrtf(aa) * sqrtf(bb)), with the correctly rounded divide and square root the compiler emits by default (this
// file gets no fast-math flag, and -ffp-contract=off keeps every multiply and add apart).  A row that is not valid is never read: the index
// checks are wave-uniform and come first.  Verdict tallies go through eight LDS integers and leave as one integer atomicAdd per counter and
// workgroup; there are no float atomics.
#include "common.h"

namespace {

constexpr int PV_THREADS = 256, PV_PAIRS = PV_THREADS / 64;

struct PVArgs {
    const float *emb;                 // [n_rows][dim]
    const int32_t *pairs;             // [P][2]
    const int32_t *offsets;           // [n_img + 1] or NULL
    const int32_t *labels;            // [P] or NULL
    float *score;                     // [P]
    int32_t *verdict;                 // [P]
    int32_t *counters;                // [8], added to
    float thresh;
    int n_rows, dim, P, n_img;
};

// One side of a pair -> its row of emb (>= 0), or -1 = no image, -2 = no face.
__device__ __forceinline__ int pv_row(const PVArgs &a, int e) {
    if (a.offsets == nullptr) return e == -1 ? -1 : ((e >= 0 && e < a.n_rows) ? e : -2);
    if (e < 0 || e >= a.n_img) return -1;
    const int o0 = a.offsets[e], o1 = a.offsets[e + 1];
    return (o1 > o0 && o0 >= 0 && o0 < a.n_rows) ? o0 : -2;
}

__global__ void __launch_bounds__(PV_THREADS) pair_verify(const PVArgs a) {
    __shared__ int tally[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = blockIdx.x * PV_PAIRS + (tid >> 6);      // wave-uniform
    if (tid < 8) tally[tid] = 0;
    __syncthreads();
    if (p < a.P) {
        const int ra = pv_row(a, a.pairs[2 * (size_t)p]), rb = pv_row(a, a.pairs[2 * (size_t)p + 1]);
        int v;
        float s = 0.f;
        if (ra == -1 || rb == -1) v = FID_PAIR_NO_IMAGE;    // the reference's order of checks: the download first (:896), then the faces (:915)
        else if (ra < 0 || rb < 0) v = FID_PAIR_NO_FACE;
        else {
            const float4 *A = (const float4 *)(a.emb + (size_t)ra * a.dim), *B = (const float4 *)(a.emb + (size_t)rb * a.dim);
            float dot = 0.f, aa = 0.f, bb = 0.f;
            const int n4 = a.dim >> 2;
            for (int i = lane; i < n4; i += 64) {
                const float4 x = A[i], y = B[i];
                dot += x.x * y.x; dot += x.y * y.y; dot += x.z * y.z; dot += x.w * y.w;
                aa += x.x * x.x; aa += x.y * x.y; aa += x.z * x.z; aa += x.w * x.w;
                bb += y.x * y.x; bb += y.y * y.y; bb += y.z * y.z; bb += y.w * y.w;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                dot += __shfl_xor(dot, o);
                aa += __shfl_xor(aa, o);
                bb += __shfl_xor(bb, o);
            }
            s = dot / (sqrtf(aa) * sqrtf(bb));              // :978; a zero row: 0 / 0 = NaN, and NaN > t is false
            v = s > a.thresh ? FID_PAIR_SAME : FID_PAIR_DIFFERENT;
        }
        if (lane == 0) {
            a.score[p] = s;
            a.verdict[p] = v;
            atomicAdd(&tally[0], 1);
            atomicAdd(&tally[v == FID_PAIR_SAME ? 1 : v == FID_PAIR_DIFFERENT ? 2 : v == FID_PAIR_NO_IMAGE ? 3 : 4], 1);
            const int lab = a.labels ? a.labels[p] : -1;
            if (lab == 0 || lab == 1) {
                atomicAdd(&tally[5], 1);
                if ((lab == 1) == (v == FID_PAIR_SAME)) atomicAdd(&tally[6], 1);   // :1082: an error pair is "not the same person"
            }
        }
    }
    __syncthreads();
    if (tid < 7 && tally[tid] != 0) atomicAdd(a.counters + tid, tally[tid]);
}

}  // namespace

extern "C" int fid_pair_verify(fid_ctx *ctx, const float *emb_dev, int n_rows, int dim, const int32_t *pairs_dev, int P,
                               const int32_t *offsets_dev, int n_img, const int32_t *labels_dev, float thresh, float *score_dev,
                               int32_t *verdict_dev, int32_t *counters_dev) {
    FID_REQUIRE(ctx, "pair_verify: NULL context");
    FID_REQUIRE(P >= 0 && n_rows >= 0 && n_img >= 0, "pair_verify: P %d, n_rows %d or n_img %d is negative", P, n_rows, n_img);
    FID_REQUIRE(dim > 0 && dim % 4 == 0, "pair_verify: embedding dim %d must be a positive multiple of 4", dim);
    FID_REQUIRE(((uintptr_t)emb_dev & 15) == 0, "pair_verify: the embedding rows must be 16-byte aligned");
    FID_REQUIRE(emb_dev || n_rows == 0, "pair_verify: NULL embeddings with n_rows %d", n_rows);
    if (P == 0) return FID_OK;
    FID_REQUIRE(pairs_dev && score_dev && verdict_dev && counters_dev, "pair_verify: NULL pair table or output pointer");
    PVArgs a{};
    a.emb = emb_dev; a.pairs = pairs_dev; a.offsets = offsets_dev; a.labels = labels_dev;
    a.score = score_dev; a.verdict = verdict_dev; a.counters = counters_dev;
    a.thresh = thresh; a.n_rows = n_rows; a.dim = dim; a.P = P; a.n_img = n_img;
    std::lock_guard<std::mutex> lk(ctx->mu);
    FID_HIP(hipSetDevice(ctx->device));            // (a thread may drive contexts on several devices)
    hipLaunchKernelGGL(pair_verify, dim3((unsigned)((P - 1) / PV_PAIRS + 1)), dim3(PV_THREADS), 0, ctx->stream, a);
    FID_HIP(hipGetLastError());
    return FID_OK;
}
