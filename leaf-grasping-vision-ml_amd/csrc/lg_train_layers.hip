// Training step, everything between the convolutions and the loss: BatchNorm2d (batch statistics, ReLU, max-pool, Dropout2d
// mask) forward and backward, spatial attention with the global average pool, the elementwise pieces of channel attention,
// the classifier's Linear and BatchNorm1d layers, and their launchers (lg_train.h).  HBM- or latency-bound elementwise /
// reduction work; all reductions are ordered, two runs give identical bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "lg_train.h"

namespace {

// Workgroups of 64 columns x kRG row groups: a row group walks rows rg, rg + kRG, ...; the kRG partial sums of a column
// are added in index order by every thread of the column.
constexpr int kRG = 16;
__device__ inline float rg_sum(float v, float (*s)[64], int f, int rg) {
    __syncthreads();
    s[rg][f] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < kRG; k++) t += s[k][f];
    return t;
}

// ------------------------------------------------------------------------------------------------ BatchNorm2d
// Workgroup (c, s) reduces channel c over sample chunk s: count, mean and M2 = sum (x - chunk mean)^2 (two passes, the
// second one hits L2).  The chunks are combined in index order with Chan's formula -- by the same workgroup when there
// is one chunk, else by lgt_bn_finish_kernel: mean, biased variance -> rstd; running statistics as nn.BatchNorm2d
// (momentum 0.1, unbiased variance in the running estimate).
__device__ inline void bn_finish(int c, float cnt, float mu, float m2, float eps, float momentum, float* mean, float* rstd,
                                 float* run_mean, float* run_var) {
    const float var = m2 / cnt;
    mean[c] = mu;
    rstd[c] = 1.0f / sqrtf(var + eps);
    run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mu;
    run_var[c] = (1.0f - momentum) * run_var[c] + momentum * var * (cnt / (cnt > 1.0f ? cnt - 1.0f : 1.0f));
}
__global__ __launch_bounds__(256) void lgt_bn_stats_kernel(const float* __restrict__ x, int N, int C, int HW, int chunk,
                                                           float eps, float momentum, float* __restrict__ part,
                                                           float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var) {
    __shared__ float s_red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int na = blockIdx.y * chunk, nb = min(N, na + chunk), M = (nb - na) * HW;
    const float* xc = x + ((size_t)na * C + c) * HW;
    const size_t sn = (size_t)C * HW;
    float s = 0.0f;
#pragma unroll 4
    for (int i = t; i < M; i += 256) s += xc[(size_t)(i / HW) * sn + i % HW];
    const float mu = block_sum(s, s_red) / (float)M;
    float v = 0.0f;
#pragma unroll 4
    for (int i = t; i < M; i += 256) {
        const float d = xc[(size_t)(i / HW) * sn + i % HW] - mu;
        v += d * d;
    }
    const float m2 = block_sum(v, s_red);
    if (t == 0) {
        if (gridDim.y == 1) bn_finish(c, (float)M, mu, m2, eps, momentum, mean, rstd, run_mean, run_var);
        else {
            float* q = part + ((size_t)c * gridDim.y + blockIdx.y) * 3;
            q[0] = (float)M; q[1] = mu; q[2] = m2;
        }
    }
}
__global__ void lgt_bn_finish_kernel(const float* __restrict__ part, int C, int S, float eps, float momentum,
                                     float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                     float* __restrict__ run_var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float* q = part + (size_t)c * S * 3;
    float cnt = q[0], mu = q[1], m2 = q[2];
    for (int k = 1; k < S; k++) {
        const float nb = q[3 * k], mb = q[3 * k + 1], d = mb - mu, tot = cnt + nb;
        mu += d * (nb / tot);
        m2 += q[3 * k + 2] + d * d * (cnt * nb / tot);
        cnt = tot;
    }
    bn_finish(c, cnt, mu, m2, eps, momentum, mean, rstd, run_mean, run_var);
}
// out[k] = sum_s part[k][s]   (k < K, fixed order)
__global__ void lgt_rowsum_kernel(const float* __restrict__ part, int K, int S, float* __restrict__ o0, float* __restrict__ o1,
                                  int K0) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    float s = 0.0f;
    for (int j = 0; j < S; j++) s += part[(size_t)k * S + j];
    if (k < K0) o0[k] = s; else o1[k - K0] = s;
}

__device__ inline float bn_relu(float x, float mu, float rs, float g, float b) { return fmaxf((x - mu) * rs * g + b, 0.0f); }

// first maximum of the 2x2 cell in row-major scan order (nn.MaxPool2d routes the gradient there)
__device__ inline int argmax4(const float y[4]) {
    int k = 0;
    float m = y[0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (y[i] > m) { m = y[i]; k = i; }
    return k;
}

// out = relu(bn(x))                                   (POOL = false)
// out = maxpool2x2(relu(bn(x))) * dmask[n][c]          (POOL = true: Dropout2d keep mask, already scaled by 1/(1-p))
template <bool POOL>
__global__ void lgt_bn_act_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                  const float* __restrict__ rstd, const float* __restrict__ gam,
                                  const float* __restrict__ bet, const float* __restrict__ dmask,
                                  float* __restrict__ out, int N, int C, int WI) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!POOL) {
        const int HW = WI * WI;
        if (idx >= (size_t)N * C * HW) return;
        const int c = (idx / HW) % C;
        out[idx] = bn_relu(x[idx], mean[c], rstd[c], gam[c], bet[c]);
    } else {
        const int WO = WI / 2;
        if (idx >= (size_t)N * C * WO * WO) return;
        const int xo = idx % WO, yo = (idx / WO) % WO;
        const size_t nc = idx / (WO * WO);
        const int c = nc % C;
        const float* xp = x + (nc * WI + 2 * yo) * WI + 2 * xo;
        const float mu = mean[c], rs = rstd[c], g = gam[c], b = bet[c];
        const float m = fmaxf(fmaxf(bn_relu(xp[0], mu, rs, g, b), bn_relu(xp[1], mu, rs, g, b)),
                              fmaxf(bn_relu(xp[WI], mu, rs, g, b), bn_relu(xp[WI + 1], mu, rs, g, b)));
        out[idx] = m * dmask[nc];
    }
}

// dgamma[c] = sum dy * xhat, dbeta[c] = sum dy with dy = dout routed back through (dropout, max-pool,) ReLU
template <bool POOL>
__global__ __launch_bounds__(256) void lgt_bn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gam, const float* __restrict__ bet,
                                                                const float* __restrict__ dmask, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, float* __restrict__ part, int chunk,
                                                                float* __restrict__ dx, int N, int C, int WI) {
    __shared__ float s_red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int na = blockIdx.y * chunk, nb = min(N, na + chunk);
    const float mu = mean[c], rs = rstd[c], g = gam[c], b = bet[c];
    float sg = 0.0f, sb = 0.0f;
    if (!POOL) {
        const int HW = WI * WI, M = (nb - na) * HW;
#pragma unroll 4
        for (int i = t; i < M; i += 256) {
            const size_t e = ((size_t)(na + i / HW) * C + c) * HW + i % HW;
            const float xh = (x[e] - mu) * rs;
            const float dy = (xh * g + b > 0.0f) ? dout[e] : 0.0f;
            sg += dy * xh;
            sb += dy;
        }
    } else {
        const int WO = WI / 2, HWO = WO * WO, M = (nb - na) * HWO;
        for (int i = t; i < M; i += 256) {
            const int n = na + i / HWO, r = i % HWO, yo = r / WO, xo = r % WO;
            const size_t nc = (size_t)n * C + c;
            const float* xp = x + (nc * WI + 2 * yo) * WI + 2 * xo;
            const float xh[4] = {(xp[0] - mu) * rs, (xp[1] - mu) * rs, (xp[WI] - mu) * rs, (xp[WI + 1] - mu) * rs};
            const float y[4] = {fmaxf(xh[0] * g + b, 0.0f), fmaxf(xh[1] * g + b, 0.0f), fmaxf(xh[2] * g + b, 0.0f),
                                fmaxf(xh[3] * g + b, 0.0f)};
            const int k = argmax4(y);
            const float dy = y[k] > 0.0f ? dout[nc * HWO + r] * dmask[nc] : 0.0f;
            sg += dy * xh[k];
            sb += dy;
        }
    }
    sg = block_sum(sg, s_red);
    sb = block_sum(sb, s_red);
    if (t == 0) {
        if (gridDim.y == 1) { dgamma[c] = sg; dbeta[c] = sb; }
        else {   // part[0..C) rows = dgamma chunks, part[C..2C) rows = dbeta chunks; summed by lgt_rowsum_kernel
            part[(size_t)c * gridDim.y + blockIdx.y] = sg;
            part[(size_t)(C + c) * gridDim.y + blockIdx.y] = sb;
        }
    }
    if (dx == nullptr || gridDim.y != 1) return;
    // small batches: the same workgroup writes dx of its channel (what lgt_bn_bwd_dx_kernel does for large ones)
    const float invM = 1.0f / (float)(N * WI * WI), mb = sb * invM, mg = sg * invM;
    if (!POOL) {
        const int HW = WI * WI, M = N * HW;
#pragma unroll 4
        for (int i = t; i < M; i += 256) {
            const size_t e = ((size_t)(i / HW) * C + c) * HW + i % HW;
            const float xh = (x[e] - mu) * rs;
            const float dy = (xh * g + b > 0.0f) ? dout[e] : 0.0f;
            dx[e] = g * rs * (dy - mb - xh * mg);
        }
    } else {
        const int WO = WI / 2, HWO = WO * WO, M = N * HWO;
        for (int i = t; i < M; i += 256) {
            const int n = i / HWO, r = i % HWO, yo = r / WO, xo = r % WO;
            const size_t nc = (size_t)n * C + c, e0 = (nc * WI + 2 * yo) * WI + 2 * xo;
            const float xh[4] = {(x[e0] - mu) * rs, (x[e0 + 1] - mu) * rs, (x[e0 + WI] - mu) * rs, (x[e0 + WI + 1] - mu) * rs};
            const float y[4] = {fmaxf(xh[0] * g + b, 0.0f), fmaxf(xh[1] * g + b, 0.0f), fmaxf(xh[2] * g + b, 0.0f),
                                fmaxf(xh[3] * g + b, 0.0f)};
            const int k = argmax4(y);
            const float dyk = y[k] > 0.0f ? dout[nc * HWO + r] * dmask[nc] : 0.0f;
            const size_t eo[4] = {e0, e0 + 1, e0 + WI, e0 + WI + 1};
#pragma unroll
            for (int q = 0; q < 4; q++) dx[eo[q]] = g * rs * ((q == k ? dyk : 0.0f) - mb - xh[q] * mg);
        }
    }
}

// dx = gamma * rstd * (dy - dbeta / M - xhat * dgamma / M)
template <bool POOL>
__global__ void lgt_bn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                     const float* __restrict__ gam, const float* __restrict__ bet,
                                     const float* __restrict__ dmask, const float* __restrict__ dgamma,
                                     const float* __restrict__ dbeta, float* __restrict__ dx, int N, int C, int WI) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float invM = 1.0f / (float)(N * WI * WI);
    if (!POOL) {
        const int HW = WI * WI;
        if (idx >= (size_t)N * C * HW) return;
        const int c = (idx / HW) % C;
        const float rs = rstd[c], g = gam[c];
        const float xh = (x[idx] - mean[c]) * rs;
        const float dy = (xh * g + bet[c] > 0.0f) ? dout[idx] : 0.0f;
        dx[idx] = g * rs * (dy - dbeta[c] * invM - xh * dgamma[c] * invM);
    } else {
        const int WO = WI / 2;
        if (idx >= (size_t)N * C * WO * WO) return;
        const int xo = idx % WO, yo = (idx / WO) % WO;
        const size_t nc = idx / (WO * WO);
        const int c = nc % C;
        const size_t e0 = (nc * WI + 2 * yo) * WI + 2 * xo;
        const float mu = mean[c], rs = rstd[c], g = gam[c], b = bet[c];
        const float xh[4] = {(x[e0] - mu) * rs, (x[e0 + 1] - mu) * rs, (x[e0 + WI] - mu) * rs, (x[e0 + WI + 1] - mu) * rs};
        const float y[4] = {fmaxf(xh[0] * g + b, 0.0f), fmaxf(xh[1] * g + b, 0.0f), fmaxf(xh[2] * g + b, 0.0f),
                            fmaxf(xh[3] * g + b, 0.0f)};
        const int k = argmax4(y);
        const float dyk = y[k] > 0.0f ? dout[idx] * dmask[nc] : 0.0f;
        const float mb = dbeta[c] * invM, mg = dgamma[c] * invM;
        const size_t eo[4] = {e0, e0 + 1, e0 + WI, e0 + WI + 1};
#pragma unroll
        for (int i = 0; i < 4; i++) dx[eo[i]] = g * rs * ((i == k ? dyk : 0.0f) - mb - xh[i] * mg);
    }
}

// ------------------------------------------------------------------------------------------------ head
// spatial attention + global average pool: a[n][p] = sigmoid(ba + sum_c wa[c] h[n][c][p]); g[n][c] = mean_p h a
__global__ __launch_bounds__(256) void lgt_att_fwd_kernel(const float* __restrict__ h, const float* __restrict__ wa,
                                                          const float* __restrict__ ba, int spatial, int F, int P,
                                                          float* __restrict__ a, float* __restrict__ g) {
    __shared__ float s_a[64], s_p[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const float* hn = h + (size_t)n * F * P;
    const int p = t % P, cg = t / P, G = 256 / P;     // P divides 256 (1, 4, 16, 64)
    float s = 0.0f;
    if (spatial)
        for (int c = cg; c < F; c += G) s += wa[c] * hn[c * P + p];
    s_p[t] = s;
    __syncthreads();
    if (t < P) {
        float v = 1.0f;
        if (spatial) {
            float z = ba[0];
            for (int k = 0; k < G; k++) z += s_p[k * P + t];
            v = 1.0f / (1.0f + expf(-z));
        }
        s_a[t] = v;
        a[(size_t)n * P + t] = v;
    }
    __syncthreads();
    for (int c = t; c < F; c += 256) {
        float z = 0.0f;
        for (int q = 0; q < P; q++) z += hn[c * P + q] * s_a[q];
        g[(size_t)n * F + c] = z / (float)P;
    }
}

// dh[n][c][p] = dg[n][c] a[p] / P + ds[p] wa[c],  ds[p] = a (1-a) sum_c dg[c] h[c][p] / P;
// part[n][c] = sum_p ds[p] h[c][p] (-> d wa),  part[n][F] = sum_p ds[p] (-> d ba)
__global__ __launch_bounds__(256) void lgt_att_bwd_kernel(const float* __restrict__ h, const float* __restrict__ a,
                                                          const float* __restrict__ dg, const float* __restrict__ wa,
                                                          int spatial, int F, int P, float* __restrict__ dh,
                                                          float* __restrict__ part, const float* __restrict__ dm) {
    __shared__ float s_a[64], s_ds[64], s_p[256];
    const int n = blockIdx.x, t = threadIdx.x;
    const float* hn = h + (size_t)n * F * P;
    const float* dgn = dg + (size_t)n * F;
    const int p = t % P, cg = t / P, G = 256 / P;
    float s = 0.0f;
    if (spatial)
        for (int c = cg; c < F; c += G) s += dgn[c] * hn[c * P + p];
    s_p[t] = s;
    __syncthreads();
    if (t < P) {
        const float av = a[(size_t)n * P + t];
        float z = 0.0f;
        for (int k = 0; k < G; k++) z += s_p[k * P + t];
        s_a[t] = av;
        s_ds[t] = spatial ? z / (float)P * av * (1.0f - av) : 0.0f;
    }
    __syncthreads();
    for (int c = t; c < F; c += 256) {
        const float d = dgn[c] / (float)P, w = spatial ? wa[c] : 0.0f;
        const float dmc = dm ? dm[(size_t)n * F + c] / (float)P : 0.0f;   // channel attention's path through mean_p h
        float pw = 0.0f;
        for (int q = 0; q < P; q++) {
            dh[((size_t)n * F + c) * P + q] = d * s_a[q] + s_ds[q] * w + dmc;
            pw += s_ds[q] * hn[c * P + q];
        }
        if (spatial) part[(size_t)n * (F + 1) + c] = pw;
    }
    if (spatial && t == 0) {
        float z = 0.0f;
        for (int q = 0; q < P; q++) z += s_ds[q];
        part[(size_t)n * (F + 1) + F] = z;
    }
}

__global__ __launch_bounds__(64 * kRG) void lgt_colsum_kernel(const float* __restrict__ part, int N, int K,
                                                              float* __restrict__ out) {
    __shared__ float s_p[kRG][64];
    const int f = threadIdx.x, rg = threadIdx.y, k = min((int)blockIdx.x * 64 + f, K - 1);
    float s = 0.0f;
    for (int n = rg; n < N; n += kRG) s += part[(size_t)n * K + k];
    s = rg_sum(s, s_p, f, rg);
    if (rg == 0 && (int)blockIdx.x * 64 + f < K) out[k] = s;
}

// Channel attention (model.py:37-44, 52-58): ca = sigmoid(W2 relu(W1 m + b1) + b2) with m = mean_p h; pooled feature
// g2 = ca * gs, gs = the (spatially attended, for 'hybrid') mean.  The two 1x1 convolutions run as the classifier's Linear
// kernels on [N][F] / [N][F/16]; these are the elementwise pieces.
__global__ void lgt_relu_kernel(const float* __restrict__ z, float* __restrict__ r, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i] = fmaxf(z[i], 0.0f);
}
__global__ void lgt_catt_gate_kernel(const float* __restrict__ z2, const float* __restrict__ gs, float* __restrict__ ca,
                                     float* __restrict__ g2, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float c = 1.0f / (1.0f + expf(-z2[i]));
    ca[i] = c;
    g2[i] = c * gs[i];
}
// dgs = dg2 * ca, dz2 = dg2 * gs * ca (1 - ca)
__global__ void lgt_catt_gate_bwd_kernel(const float* __restrict__ dg2, const float* __restrict__ ca,
                                         const float* __restrict__ gs, float* __restrict__ dgs, float* __restrict__ dz2,
                                         size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float c = ca[i], d = dg2[i];
    dgs[i] = d * c;
    dz2[i] = d * gs[i] * c * (1.0f - c);
}
// dz1 = dr * (z1 > 0)
__global__ void lgt_relu_bwd_kernel(const float* __restrict__ dr, const float* __restrict__ z1, float* __restrict__ dz1,
                                    size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dz1[i] = z1[i] > 0.0f ? dr[i] : 0.0f;
}

// Y[n][o] = b[o] + sum_i X[n][i] W[o][i]; one wave per (o, kFcRows samples), the weight row held in registers (I <= 1024).
// Four samples per wave: one dependent round of loads + shuffles per launch (16 per wave cost 18 us at batch 16).
constexpr int kFcRows = 4;
__global__ __launch_bounds__(256) void lgt_fc_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                         const float* __restrict__ b, float* __restrict__ Y, int N, int I,
                                                         int O) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= O) return;
    float w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = lane + 64 * k < I ? W[(size_t)o * I + lane + 64 * k] : 0.0f;
    const float bo = b[o];
    const int nk = (I + 63) / 64;
    const int nb = blockIdx.y * kFcRows, ne = min(N, nb + kFcRows);
    for (int n = nb; n < ne; n += 4) {   // four independent samples at a time: their loads and shuffle chains overlap
        float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k < nk && n + u < ne) s4[u] += (lane + 64 * k < I ? X[(size_t)(n + u) * I + lane + 64 * k] : 0.0f) * w[k];
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) s4[u] += __shfl_xor(s4[u], k, 64);
            if (lane == 0 && n + u < ne) Y[(size_t)(n + u) * O + o] = s4[u] + bo;
        }
    }
}

// BatchNorm1d (batch statistics) + ReLU + Dropout keep mask.  Workgroup = 64 features x kRG row groups over the samples.
__global__ __launch_bounds__(64 * kRG) void lgt_bn1d_fwd_kernel(const float* __restrict__ U, const float* __restrict__ gam,
                                    const float* __restrict__ bet, const float* __restrict__ mask, float* __restrict__ Y,
                                    float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                    float* __restrict__ run_var, int N, int O, float eps, float momentum) {
    __shared__ float s_p[kRG][64];
    const int f = threadIdx.x, rg = threadIdx.y, o = min((int)blockIdx.x * 64 + f, O - 1);
    const bool own = (int)blockIdx.x * 64 + f < O;
    float s = 0.0f;
    for (int n = rg; n < N; n += kRG) s += U[(size_t)n * O + o];
    const float mu = rg_sum(s, s_p, f, rg) / (float)N;
    float v = 0.0f;
    for (int n = rg; n < N; n += kRG) {
        const float d = U[(size_t)n * O + o] - mu;
        v += d * d;
    }
    const float var = rg_sum(v, s_p, f, rg) / (float)N, rs = 1.0f / sqrtf(var + eps);
    if (!own) return;
    if (rg == 0) {
        mean[o] = mu;
        rstd[o] = rs;
        run_mean[o] = (1.0f - momentum) * run_mean[o] + momentum * mu;
        run_var[o] = (1.0f - momentum) * run_var[o] + momentum * var * ((float)N / (float)(N > 1 ? N - 1 : 1));
    }
    const float g = gam[o], b = bet[o];
    for (int n = rg; n < N; n += kRG)
        Y[(size_t)n * O + o] = fmaxf((U[(size_t)n * O + o] - mu) * rs * g + b, 0.0f) * mask[(size_t)n * O + o];
}

__global__ __launch_bounds__(64 * kRG) void lgt_bn1d_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ U,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const float* __restrict__ gam, const float* __restrict__ bet,
                                    const float* __restrict__ mask, float* __restrict__ dU, float* __restrict__ dgamma,
                                    float* __restrict__ dbeta, int N, int O) {
    __shared__ float s_p[kRG][64];
    const int f = threadIdx.x, rg = threadIdx.y, o = min((int)blockIdx.x * 64 + f, O - 1);
    const bool own = (int)blockIdx.x * 64 + f < O;
    const float mu = mean[o], rs = rstd[o], g = gam[o], b = bet[o];
    float sg = 0.0f, sb = 0.0f;
    for (int n = rg; n < N; n += kRG) {
        const float xh = (U[(size_t)n * O + o] - mu) * rs;
        const float dy = (xh * g + b > 0.0f) ? dY[(size_t)n * O + o] * mask[(size_t)n * O + o] : 0.0f;
        sg += dy * xh;
        sb += dy;
    }
    sg = rg_sum(sg, s_p, f, rg);
    sb = rg_sum(sb, s_p, f, rg);
    if (!own) return;
    if (rg == 0) { dgamma[o] = sg; dbeta[o] = sb; }
    const float invN = 1.0f / (float)N;
    for (int n = rg; n < N; n += kRG) {
        const float xh = (U[(size_t)n * O + o] - mu) * rs;
        const float dy = (xh * g + b > 0.0f) ? dY[(size_t)n * O + o] * mask[(size_t)n * O + o] : 0.0f;
        dU[(size_t)n * O + o] = g * rs * (dy - sb * invN - xh * sg * invN);
    }
}

// dX[n][i] = sum_o dY[n][o] W[o][i]
__global__ __launch_bounds__(64 * kRG) void lgt_fc_bwd_x_kernel(const float* __restrict__ dY, const float* __restrict__ W,
                                                                float* __restrict__ dX, int N, int I, int O) {
    __shared__ float s_p[kRG][64];
    const int f = threadIdx.x, rg = threadIdx.y, i = min((int)blockIdx.x * 64 + f, I - 1), n = blockIdx.y;
    float s = 0.0f;
    for (int o = rg; o < O; o += kRG) s += dY[(size_t)n * O + o] * W[(size_t)o * I + i];
    s = rg_sum(s, s_p, f, rg);
    if (rg == 0 && (int)blockIdx.x * 64 + f < I) dX[(size_t)n * I + i] = s;
}

// dW[o][i] = sum_n dY[n][o] X[n][i], db[o] = sum_n dY[n][o]
__global__ __launch_bounds__(64 * kRG) void lgt_fc_bwd_w_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                                float* __restrict__ dW, float* __restrict__ db, int N, int I,
                                                                int O) {
    __shared__ float s_p[kRG][64];
    const int f = threadIdx.x, rg = threadIdx.y, i = min((int)blockIdx.x * 64 + f, I - 1), o = blockIdx.y;
    float s = 0.0f, sb = 0.0f;
    for (int n = rg; n < N; n += kRG) {
        const float d = dY[(size_t)n * O + o];
        s += d * X[(size_t)n * I + i];
        sb += d;
    }
    s = rg_sum(s, s_p, f, rg);
    sb = rg_sum(sb, s_p, f, rg);
    if (rg == 0 && (int)blockIdx.x * 64 + f < I) dW[(size_t)o * I + i] = s;
    if (rg == 0 && f == 0 && blockIdx.x == 0) db[o] = sb;
}

constexpr int kBnSplit = 64;                    // BatchNorm reduction: sample chunks per channel
// sample chunks of the BatchNorm reductions: about 4096 elements per workgroup, at most 2048 workgroups, never more
// chunks than samples (batch 16 at 32x32: 4 chunks instead of one workgroup walking 16384 elements three times)
int bn_chunks(int N, int C, int HW) {
    const long long M = (long long)N * HW;
    const int want = (int)std::min<long long>(M / 4096, (long long)kBnSplit);
    return std::max(1, std::min(std::min(want, N), std::max(1, 2048 / C)));
}
// the y extent of both reduction grids: samples per chunk, chunks that hold a sample
struct BnGrid { int chunk, Sy; };
BnGrid bn_grid(int N, int C, int HW) {
    const int S = bn_chunks(N, C, HW), chunk = (N + S - 1) / S;
    return {chunk, (N + chunk - 1) / chunk};
}
constexpr int att_part_cols(int F) { return F + 1; }   // lgt_att_bwd_kernel's row of part: d wa [F], d ba

// the kernel's <true> instantiation when `pool`, else <false>
#define LGT_POOL_LAUNCH(kernel, pool, ...)                       \
    do {                                                         \
        if (pool) hipLaunchKernelGGL(kernel<true>, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<false>, __VA_ARGS__);     \
    } while (0)

}  // namespace

size_t lgt_bn_part_floats() { return (size_t)kLgtMaxChannels * kBnSplit * 3; }   // forward: 3 per (channel, chunk); backward: 2
void lgt_bn2d_fwd(const float* x, const float* gam, const float* bet, const float* dmask, float* part, float* mean, float* rstd,
                  float* run_mean, float* run_var, float* out, int N, int C, int wi, float eps, float momentum, hipStream_t s) {
    const BnGrid g = bn_grid(N, C, wi * wi);
    hipLaunchKernelGGL(lgt_bn_stats_kernel, dim3(C, g.Sy), dim3(256), 0, s, x, N, C, wi * wi, g.chunk, eps, momentum, part, mean,
                       rstd, run_mean, run_var);
    if (g.Sy > 1)
        hipLaunchKernelGGL(lgt_bn_finish_kernel, dim3(lgt_cdiv(C, 64)), dim3(64), 0, s, part, C, g.Sy, eps, momentum,
                           mean, rstd, run_mean, run_var);
    const bool pool = dmask != nullptr;
    const size_t n = (size_t)N * C * wi * wi / (pool ? 4 : 1);
    LGT_POOL_LAUNCH(lgt_bn_act_kernel, pool, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, x, mean, rstd,
                    gam, bet, dmask, out, N, C, wi);
}
void lgt_bn2d_bwd(const float* x, const float* dout, const float* mean, const float* rstd, const float* gam, const float* bet,
                  const float* dmask, float* dgamma, float* dbeta, float* part, float* dx, int N, int C, int wi, hipStream_t s) {
    const BnGrid g = bn_grid(N, C, wi * wi);
    const bool pool = dmask != nullptr;
    LGT_POOL_LAUNCH(lgt_bn_bwd_reduce_kernel, pool, dim3(C, g.Sy), dim3(256), 0, s, x, dout, mean, rstd, gam, bet, dmask, dgamma,
                    dbeta, part, g.chunk, dx, N, C, wi);
    if (g.Sy > 1) {   // large batches: ordered sum of the chunks, then dx over the whole chip
        hipLaunchKernelGGL(lgt_rowsum_kernel, dim3(lgt_cdiv(2 * C, 64)), dim3(64), 0, s, part, 2 * C, g.Sy, dgamma,
                           dbeta, C);
        const size_t n = (size_t)N * C * wi * wi / (pool ? 4 : 1);
        LGT_POOL_LAUNCH(lgt_bn_bwd_dx_kernel, pool, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, x, dout, mean, rstd, gam, bet, dmask,
                        dgamma, dbeta, dx, N, C, wi);
    }
}

void lgt_att_fwd(const float* h, const float* wa, const float* ba, int spatial, int N, int F, int P, float* a, float* g,
                 hipStream_t s) {
    hipLaunchKernelGGL(lgt_att_fwd_kernel, dim3(N), dim3(256), 0, s, h, wa, ba, spatial, F, P, a, g);
}
size_t lgt_att_part_floats(int N, int F) { return (size_t)N * att_part_cols(F); }
void lgt_att_bwd(const float* h, const float* a, const float* dg, const float* wa, int spatial, int N, int F, int P, float* dh,
                 float* part, const float* dm, float* dwab, hipStream_t s) {
    hipLaunchKernelGGL(lgt_att_bwd_kernel, dim3(N), dim3(256), 0, s, h, a, dg, wa, spatial, F, P, dh, part, dm);
    if (spatial)
        hipLaunchKernelGGL(lgt_colsum_kernel, dim3(lgt_cdiv(att_part_cols(F), 64)), dim3(64, kRG), 0, s, part, N,
                           att_part_cols(F), dwab);
}

void lgt_fc_fwd(const float* X, const float* W, const float* b, float* Y, int N, int I, int O, hipStream_t s) {
    hipLaunchKernelGGL(lgt_fc_fwd_kernel, dim3(lgt_cdiv(O, 4), lgt_cdiv(N, kFcRows)), dim3(256), 0, s, X, W, b, Y, N, I, O);
}
void lgt_fc_bwd(const float* dY, const float* X, const float* W, float* dW, float* db, float* dX, int N, int I, int O,
                hipStream_t s) {
    hipLaunchKernelGGL(lgt_fc_bwd_w_kernel, dim3(lgt_cdiv(I, 64), O), dim3(64, kRG), 0, s, dY, X, dW, db, N, I, O);
    hipLaunchKernelGGL(lgt_fc_bwd_x_kernel, dim3(lgt_cdiv(I, 64), N), dim3(64, kRG), 0, s, dY, W, dX, N, I, O);
}
void lgt_bn1d_fwd(const float* U, const float* gam, const float* bet, const float* mask, float* Y, float* mean, float* rstd,
                  float* run_mean, float* run_var, int N, int O, float eps, float momentum, hipStream_t s) {
    hipLaunchKernelGGL(lgt_bn1d_fwd_kernel, dim3(lgt_cdiv(O, 64)), dim3(64, kRG), 0, s, U, gam, bet, mask, Y, mean, rstd, run_mean,
                       run_var, N, O, eps, momentum);
}
void lgt_bn1d_bwd(const float* dY, const float* U, const float* mean, const float* rstd, const float* gam, const float* bet,
                  const float* mask, float* dU, float* dgamma, float* dbeta, int N, int O, hipStream_t s) {
    hipLaunchKernelGGL(lgt_bn1d_bwd_kernel, dim3(lgt_cdiv(O, 64)), dim3(64, kRG), 0, s, dY, U, mean, rstd, gam, bet, mask, dU,
                       dgamma, dbeta, N, O);
}

void lgt_relu_fwd(const float* z, float* r, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(lgt_relu_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, z, r, n);
}
void lgt_relu_bwd(const float* dr, const float* z1, float* dz1, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(lgt_relu_bwd_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, dr, z1, dz1, n);
}
void lgt_catt_gate_fwd(const float* z2, const float* gs, float* ca, float* g2, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(lgt_catt_gate_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, z2, gs, ca, g2, n);
}
void lgt_catt_gate_bwd(const float* dg2, const float* ca, const float* gs, float* dgs, float* dz2, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(lgt_catt_gate_bwd_kernel, dim3(lgt_cdiv(n, 256)), dim3(256), 0, s, dg2, ca, gs, dgs, dz2, n);
}
