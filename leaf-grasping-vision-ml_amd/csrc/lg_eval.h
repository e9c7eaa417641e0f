// Validation metrics of a labelled set from its logits (scripts/train_model.py:280-298 + analyze_predictions :64-99): the
// per-sample term and the chunk walk are one piece of code that the host twin (lg_eval_logits_host) and the device kernels run.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/leafgrasp.h"

// BCEWithLogitsLoss(pos_weight) of one sample in double (lgt_loss_kernel's formula, widened):
// (1 - y) z + (1 + (pw - 1) y) (max(-z, 0) + log1p(exp(-|z|)))
__host__ __device__ inline double lg_eval_term(float z_, float y_, double pw) {
    const double z = (double)z_, y = (double)y_;
    return (1.0 - y) * z + (1.0 + (pw - 1.0) * y) * (fmax(-z, 0.0) + log1p(exp(-fabs(z))));
}

struct LgEvalChunk {   // one chunk of the walk
    double mean;                         // its terms added in index order / its length
    int tp, tn, pos, neg, correct;       // pred = z > threshold (float compare); correct: (z > 0) == (y == 1)
    int pad_;
};

// chunk c = samples [c * chunk, min(N, (c + 1) * chunk))
__host__ __device__ inline LgEvalChunk lg_eval_chunk(const float* logits, const float* labels, int N, int chunk, long long c,
                                                     double pw, float threshold) {
    const long long i0 = c * chunk, i1 = i0 + chunk < N ? i0 + chunk : N;
    LgEvalChunk r = {0.0, 0, 0, 0, 0, 0, 0};
    double sum = 0.0;
    for (long long i = i0; i < i1; i++) {
        const float z = logits[i], y = labels[i];
        sum += lg_eval_term(z, y, pw);
        const bool pred = z > threshold;
        r.tp += pred && y == 1.0f;
        r.tn += !pred && y == 0.0f;
        r.pos += y == 1.0f;
        r.neg += y == 0.0f;
        r.correct += (z > 0.0f) == (y == 1.0f);
    }
    r.mean = sum / (double)(i1 - i0);
    return r;
}

// the chunks in order -> the result (chunk means added in chunk order / n_chunks)
__host__ __device__ inline void lg_eval_add(lg_eval_result* out, double* loss_sum, const LgEvalChunk& r) {
    *loss_sum += r.mean;
    out->tp += r.tp; out->tn += r.tn;
    out->fp += r.neg - r.tn;
    out->fn += r.pos - r.tp;
    out->correct += r.correct;
}

// bytes of device scratch lg_eval_enqueue needs for N samples in chunks of `chunk`
size_t lg_eval_scratch_bytes(int N, int chunk);
// logits, labels DEVICE [N]; scratch DEVICE (lg_eval_scratch_bytes); the result is written to the first sizeof(lg_eval_result)
// bytes of scratch by the last of two launches on s
void lg_eval_enqueue(const float* logits, const float* labels, int N, int chunk, double pw, float threshold, void* scratch,
                     hipStream_t s);
