// Training step, what stands around the layers: BCEWithLogits(pos_weight) loss, global-norm gradient clipping and Adam with
// L2 weight decay, the dropout keep masks drawn on the device, the gather and filing kernels of lg_train_epoch, and their
// launchers (lg_train.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lg_train.h"

namespace {

// BCEWithLogitsLoss(pos_weight), mean over the batch (train_model.py:221,251): loss and d loss / d logit
__global__ __launch_bounds__(256) void lgt_loss_kernel(const float* __restrict__ z, const float* __restrict__ y, int N,
                                                       const AdamHp* __restrict__ hp, float* __restrict__ loss,
                                                       float* __restrict__ dz) {
    __shared__ float s_red[4];
    const float pos_weight = hp->pos_weight;
    float s = 0.0f;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float zn = z[n], yn = y[n];
        // (1 - y) z + lw softplus(-z), lw = 1 + (pos_weight - 1) y, written as (1 - y) softplus(z) + pos_weight y softplus(-z):
        // the same number without z + softplus(-z), which cancels to nothing at z << 0 (z = -20: 0 instead of 2e-9).
        // softplus(+-z) = max(+-z, 0) + log1p(exp(-|z|)).  Likewise (1 - y) - lw (1 - sigmoid(z)) =
        // (1 - y) sigmoid(z) - pos_weight y sigmoid(-z), each sigmoid from exp(-|z|) <= 1.
        const float e = expf(-fabsf(zn)), l1p = log1pf(e);
        const float sp_pos = fmaxf(zn, 0.0f) + l1p, sp_neg = fmaxf(-zn, 0.0f) + l1p;
        s += (1.0f - yn) * sp_pos + pos_weight * yn * sp_neg;
        const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);   // sigmoid(|z|), sigmoid(-|z|)
        const float sig_pos = zn >= 0.0f ? big : small, sig_neg = zn >= 0.0f ? small : big;
        dz[n] = ((1.0f - yn) * sig_pos - pos_weight * yn * sig_neg) / (float)N;
    }
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) loss[0] = s / (float)N;
}

// ------------------------------------------------------------------------------------------------ optimizer
__global__ __launch_bounds__(256) void lgt_sumsq_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partial) {
    __shared__ float s_red[4];
    float s = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += g[i] * g[i];
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}


// state[0] = step count (float), state[1] = total gradient norm of this step (before clipping).  One wave adds the
// partial sums in index order and advances the step count when the optimizer runs.
__global__ __launch_bounds__(64) void lgt_norm_kernel(const float* __restrict__ partial, int nparts, int advance,
                                                      float* __restrict__ state) {
    float ss = 0.0f;   // one wave: lane l adds partials l, l + 64, ... in order, then a fixed butterfly
    for (int k = threadIdx.x; k < nparts; k += 64) ss += partial[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (threadIdx.x == 0) {
        state[1] = sqrtf(ss);
        if (advance) state[0] += 1.0f;
    }
}
// clip_grad_norm_(max_norm) + torch.optim.Adam(weight_decay = L2 added to the gradient)
__global__ __launch_bounds__(256) void lgt_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, size_t n,
                                                       const AdamHp* __restrict__ hp_, const float* __restrict__ state) {
    const AdamHp hp = *hp_;
    const float norm = state[1], step = state[0];
    const float coef = hp.max_norm > 0.0f ? fminf(hp.max_norm / (norm + 1e-6f), 1.0f) : 1.0f;
    const float bc1 = 1.0f - powf(hp.beta1, step), bc2 = 1.0f - powf(hp.beta2, step);
    const float step_size = hp.lr / bc1, bc2s = sqrtf(bc2);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        // torch's order, written out instead of left to the compiler's contraction: clip_grad_norm_ stores the clipped
        // gradient as a float32 tensor (one rounding), then grad.add(param, alpha = weight_decay)
        const float gi = fmaf(hp.weight_decay, p[i], __fmul_rn(g[i], coef));
        const float mi = hp.beta1 * m[i] + (1.0f - hp.beta1) * gi;
        const float vi = hp.beta2 * v[i] + (1.0f - hp.beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * (mi / (sqrtf(vi) / bc2s + hp.eps));
    }
}

// keep masks of all dropout layers in one launch: 0 or 1/(1-p); counter-based hash of (seed, index)
__global__ void lgt_mask_kernel(float* __restrict__ mask, MaskTable T, const uint64_t* __restrict__ seed_,
                                const float* __restrict__ state) {
    const uint64_t seed = seed_[0] * 0x100000001B3ull + 0x51ull * (uint64_t)state[0];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int l = 0;
    while (l < T.n && i >= T.end[l]) l++;
    if (l >= T.n) return;
    uint64_t zz = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    zz ^= zz >> 31;
    const float u = (float)(zz >> 40) * (1.0f / 16777216.0f), p = T.p[l];
    mask[i] = u >= p ? 1.0f / (1.0f - p) : 0.0f;
}

// ------------------------------------------------------------------------------------------------ device epoch
constexpr int kRowVec = 9 * 1024 / 4;   // one sample [9][32][32] as 16-byte pieces
// One step's batch straight into the step's input buffers: row r of xin / lab is sample idx[r] of the training set.
// grid (N, kRowVec / 256), one 16-byte load and store per thread; the host has checked every index against the set.
__global__ __launch_bounds__(256) void lgt_gather_kernel(const float4* __restrict__ x, const float* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, float4* __restrict__ xin,
                                                         float* __restrict__ lab) {
    const int r = blockIdx.x;
    const size_t src = (size_t)idx[r];
    const int v = blockIdx.y * 256 + threadIdx.x;
    xin[(size_t)r * kRowVec + v] = x[src * kRowVec + v];
    if (v == 0) lab[r] = labels[src];
}

// What the host reads after a step, filed on the device instead: loss and gradient norm into slot k, the step's correct
// predictions ((logit > 0) == (label == 1)) added to the epoch's counter, the logits behind those of the steps before.
// One workgroup; the steps of an epoch are in stream order, so the counter needs no atomic.
__global__ __launch_bounds__(256) void lgt_file_step_kernel(const float* __restrict__ loss, const float* __restrict__ state,
                                                            const float* __restrict__ logits, const float* __restrict__ lab,
                                                            int N, int k, float* __restrict__ losses,
                                                            float* __restrict__ grad_norms,
                                                            unsigned long long* __restrict__ correct,
                                                            float* __restrict__ logits_out) {
    __shared__ float s_red[4];
    float c = 0.0f;   // a count of at most N <= 8192: exact in float
    for (int n = threadIdx.x; n < N; n += 256) {
        const float z = logits[n];
        c += ((z > 0.0f) == (lab[n] == 1.0f)) ? 1.0f : 0.0f;
        if (logits_out) logits_out[n] = z;
    }
    c = block_sum(c, s_red);
    if (threadIdx.x == 0) {
        losses[k] = loss[0];
        grad_norms[k] = state[1];
        correct[0] += (unsigned long long)c;
    }
}

constexpr int kNormParts = 256;   // workgroups of lgt_sumsq_kernel = partial sums lgt_norm_kernel adds

}  // namespace

void lgt_draw_masks(float* mask, const MaskTable& table, const uint64_t* seed, const float* state, hipStream_t s) {
    const size_t n = table.n ? table.end[table.n - 1] : 0;
    hipLaunchKernelGGL(lgt_mask_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, mask, table, seed, state);
}
void lgt_loss(const float* z, const float* y, int N, const AdamHp* hp, float* loss, float* dz, hipStream_t s) {
    hipLaunchKernelGGL(lgt_loss_kernel, dim3(1), dim3(256), 0, s, z, y, N, hp, loss, dz);
}

size_t lgt_norm_part_floats() { return kNormParts; }
void lgt_clip_adam(const float* G, size_t n, float* P, float* M, float* V, const AdamHp* hp, float* state, float* norm_part,
                   int apply_update, hipStream_t s) {
    hipLaunchKernelGGL(lgt_sumsq_kernel, dim3(kNormParts), dim3(256), 0, s, G, n, norm_part);
    hipLaunchKernelGGL(lgt_norm_kernel, dim3(1), dim3(64), 0, s, norm_part, kNormParts, apply_update ? 1 : 0, state);
    if (apply_update) hipLaunchKernelGGL(lgt_adam_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, P, G, M, V, n, hp, state);
}

void lgt_gather_batch(const float* x, const float* labels, const int32_t* idx, int N, float* xin, float* lab, hipStream_t s) {
    hipLaunchKernelGGL(lgt_gather_kernel, dim3(N, kRowVec / 256), dim3(256), 0, s, (const float4*)x, labels, idx, (float4*)xin, lab);
}
void lgt_file_step(const float* loss, const float* state, const float* logits, const float* lab, int N, int k, float* losses,
                   float* grad_norms, unsigned long long* correct, float* logits_out, hipStream_t s) {
    hipLaunchKernelGGL(lgt_file_step_kernel, dim3(1), dim3(256), 0, s, loss, state, logits, lab, N, k, losses, grad_norms, correct,
                       logits_out);
}
