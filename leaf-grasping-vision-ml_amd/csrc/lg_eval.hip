// Validation loss and confusion counts on the device: one thread walks one chunk (lg_eval_chunk, the host twin's code), one
// workgroup then adds the chunks -- counts as integers in any order, the chunk means by one thread in chunk order, so the
// result does not depend on the grid and two runs give the same bits.  No float atomics.
#include "lg_eval.h"

namespace {

__global__ void lg_eval_chunk_kernel(const float* __restrict__ logits, const float* __restrict__ labels, int N, int chunk,
                                     long long n_chunks, double pw, float threshold, LgEvalChunk* __restrict__ part) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_chunks) part[c] = lg_eval_chunk(logits, labels, N, chunk, c, pw, threshold);
}

__global__ void lg_eval_sum_kernel(const LgEvalChunk* __restrict__ part, long long n_chunks, int N, lg_eval_result* __restrict__ out) {
    __shared__ unsigned long long cnt[5];   // tp, tn, pos, neg, correct
    if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a[5] = {0, 0, 0, 0, 0};
    for (long long c = threadIdx.x; c < n_chunks; c += blockDim.x) {
        const LgEvalChunk r = part[c];
        a[0] += r.tp; a[1] += r.tn; a[2] += r.pos; a[3] += r.neg; a[4] += r.correct;
    }
    for (int k = 0; k < 5; k++) atomicAdd(&cnt[k], a[k]);
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (long long c = 0; c < n_chunks; c++) sum += part[c].mean;
        lg_eval_result r;
        r.loss = sum / (double)n_chunks;
        r.n = N; r.n_chunks = n_chunks;
        r.correct = (int64_t)cnt[4];
        r.tp = (int64_t)cnt[0]; r.tn = (int64_t)cnt[1];
        r.fp = (int64_t)(cnt[3] - cnt[1]);
        r.fn = (int64_t)(cnt[2] - cnt[0]);
        *out = r;
    }
}

}  // namespace

static inline long long eval_chunks(int N, int chunk) { return ((long long)N + chunk - 1) / chunk; }

size_t lg_eval_scratch_bytes(int N, int chunk) { return 64 + (size_t)eval_chunks(N, chunk) * sizeof(LgEvalChunk); }

void lg_eval_enqueue(const float* logits, const float* labels, int N, int chunk, double pw, float threshold, void* scratch,
                     hipStream_t s) {
    const long long nc = eval_chunks(N, chunk);
    LgEvalChunk* part = (LgEvalChunk*)((char*)scratch + 64);
    hipLaunchKernelGGL(lg_eval_chunk_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, logits, labels, N, chunk, nc, pw,
                       threshold, part);
    hipLaunchKernelGGL(lg_eval_sum_kernel, dim3(1), dim3(256), 0, s, (const LgEvalChunk*)part, nc, N, (lg_eval_result*)scratch);
}

extern "C" int lg_eval_logits_host(const float* logits, const float* labels, int N, int chunk, double pos_weight, float threshold,
                                   lg_eval_result* out) {
    if (!logits || !labels || !out || N < 1 || chunk < 1) return LG_ERR_INVALID;
    const long long nc = eval_chunks(N, chunk);
    lg_eval_result r = {0.0, N, nc, 0, 0, 0, 0, 0};
    double sum = 0.0;
    for (long long c = 0; c < nc; c++) lg_eval_add(&r, &sum, lg_eval_chunk(logits, labels, N, chunk, c, pos_weight, threshold));
    r.loss = sum / (double)nc;
    *out = r;
    return LG_OK;
}
