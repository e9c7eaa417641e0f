// Training step (lg_train.hip): launchers of its kernels by layer type (lg_train_conv.hip, lg_train_layers.hip,
// lg_train_optim.hip), the sizes of the scratch buffers those launches write, and the three structs the host fills.
// A launcher takes plain device pointers, sizes and a stream -- never the trainer's handle --, issues its kernels in a fixed
// order and contains the branches that choose among them; it reports nothing (the caller reads hipGetLastError).  A sizing
// function stands beside the launcher whose grid it follows and shares that launcher's arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef LG_LOCAL
#define LG_LOCAL __attribute__((visibility("hidden")))
#endif

constexpr int kLgtMaxChannels = 1024;   // widest encoder block lg_train_create accepts

inline unsigned lgt_cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

#ifdef __HIPCC__
__device__ inline float block_sum(float v, float* s_red) {   // 256 threads; result in every thread
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
#endif

// ---- convolutions (lg_train_conv.hip); wi = 32 | 16 | 8 | 4: width = height of the layer's maps
// all conv layers of a step: w[l] [co][ci][tap] -> wpf[l] (forward) and wpd[l] (backward-data); end[l] = weights up to and with l
struct PackTable { const float* w[8]; float* wpf[8]; float* wpd[8]; int ci[8], co[8]; unsigned end[8]; int n; };
LG_LOCAL void lgt_pack(const PackTable& table, hipStream_t s);
// workgroups of a shape below which the next smaller shape is launched (LG_TRAIN_CONV_SMALL / LG_TRAIN_CONV_SPLIT)
struct LgtConvCut { int small_below = 256, split_below = 256; };
// out = bias + conv3x3(in, wp): forward with wpf, backward-data with dX, wpd, no bias and CI / CO swapped
LG_LOCAL void lgt_conv(LgtConvCut cut, int wi, const float* in, const float* wp, const float* bias, float* out, int N, int CI,
                       int CO, hipStream_t s);
// gw [CO][CI][9] = backward-weights of activations a [N][CI] against dx [N][CO]: partial sums per pixel slice, then their
// ordered sum.  partial holds lgt_wgrad_partial_floats(wi, N', CI, CO) floats for some N' >= N.
LG_LOCAL void lgt_wgrad(int wi, const float* a, const float* dx, float* partial, float* gw, int N, int CI, int CO, hipStream_t s);
LG_LOCAL size_t lgt_wgrad_partial_floats(int wi, int N, int CI, int CO);

// ---- BatchNorm2d, attention, classifier (lg_train_layers.hip)
// out = relu(bn(x)), or with dmask [N][C] != NULL maxpool2x2(relu(bn(x))) * dmask; batch statistics into mean / rstd, running
// statistics updated.  part: lgt_bn_part_floats() floats, also for lgt_bn2d_bwd.
LG_LOCAL void lgt_bn2d_fwd(const float* x, const float* gam, const float* bet, const float* dmask, float* part, float* mean,
                           float* rstd, float* run_mean, float* run_var, float* out, int N, int C, int wi, float eps,
                           float momentum, hipStream_t s);
// dout (at the layer's output; dmask as in the forward) -> dgamma, dbeta, dx at the convolution's output
LG_LOCAL void lgt_bn2d_bwd(const float* x, const float* dout, const float* mean, const float* rstd, const float* gam,
                           const float* bet, const float* dmask, float* dgamma, float* dbeta, float* part, float* dx, int N, int C,
                           int wi, hipStream_t s);
LG_LOCAL size_t lgt_bn_part_floats();
// a [N][P] = spatial attention map (ones when !spatial), g [N][F] = mean_p h a
LG_LOCAL void lgt_att_fwd(const float* h, const float* wa, const float* ba, int spatial, int N, int F, int P, float* a, float* g,
                          hipStream_t s);
// dg [N][F] (and dm [N][F] or NULL: channel attention's path through the plain mean) -> dh; when spatial, d wa and d ba into
// dwab [F + 1].  part: lgt_att_part_floats(N, F) floats.
LG_LOCAL void lgt_att_bwd(const float* h, const float* a, const float* dg, const float* wa, int spatial, int N, int F, int P,
                          float* dh, float* part, const float* dm, float* dwab, hipStream_t s);
LG_LOCAL size_t lgt_att_part_floats(int N, int F);
// Y [N][O] = X [N][I] W^T + b;  dW, db, then dX from dY
LG_LOCAL void lgt_fc_fwd(const float* X, const float* W, const float* b, float* Y, int N, int I, int O, hipStream_t s);
LG_LOCAL void lgt_fc_bwd(const float* dY, const float* X, const float* W, float* dW, float* db, float* dX, int N, int I, int O,
                         hipStream_t s);
// Y = relu(bn1d(U)) * mask and back
LG_LOCAL void lgt_bn1d_fwd(const float* U, const float* gam, const float* bet, const float* mask, float* Y, float* mean,
                           float* rstd, float* run_mean, float* run_var, int N, int O, float eps, float momentum, hipStream_t s);
LG_LOCAL void lgt_bn1d_bwd(const float* dY, const float* U, const float* mean, const float* rstd, const float* gam,
                           const float* bet, const float* mask, float* dU, float* dgamma, float* dbeta, int N, int O, hipStream_t s);
LG_LOCAL void lgt_relu_fwd(const float* z, float* r, size_t n, hipStream_t s);
LG_LOCAL void lgt_relu_bwd(const float* dr, const float* z1, float* dz1, size_t n, hipStream_t s);
// ca = sigmoid(z2), g2 = ca * gs;  dgs, dz2 from dg2
LG_LOCAL void lgt_catt_gate_fwd(const float* z2, const float* gs, float* ca, float* g2, size_t n, hipStream_t s);
LG_LOCAL void lgt_catt_gate_bwd(const float* dg2, const float* ca, const float* gs, float* dgs, float* dz2, size_t n, hipStream_t s);

// ---- loss, optimiser, masks, device epoch (lg_train_optim.hip)
// hyper-parameters of a step, refreshed on the device before every step (outside the captured graph)
struct AdamHp { float lr, beta1, beta2, eps, weight_decay, max_norm, pos_weight, pad; };
// the dropout layers' keep masks of a step, one behind the other: end[l] = floats up to and with layer l, p[l] its drop rate
struct MaskTable { size_t end[8]; float p[8]; int n; };
LG_LOCAL void lgt_draw_masks(float* mask, const MaskTable& table, const uint64_t* seed, const float* state, hipStream_t s);
LG_LOCAL void lgt_loss(const float* z, const float* y, int N, const AdamHp* hp, float* loss, float* dz, hipStream_t s);
// state[1] = |G|; when apply_update: state[0] += 1, clip to hp->max_norm and Adam.  norm_part: lgt_norm_part_floats() floats.
LG_LOCAL void lgt_clip_adam(const float* G, size_t n, float* P, float* M, float* V, const AdamHp* hp, float* state,
                            float* norm_part, int apply_update, hipStream_t s);
LG_LOCAL size_t lgt_norm_part_floats();
// rows idx[0..N) of the set x [.][9][32][32] (16-byte aligned), labels -> xin, lab
LG_LOCAL void lgt_gather_batch(const float* x, const float* labels, const int32_t* idx, int N, float* xin, float* lab,
                               hipStream_t s);
// step k of an epoch: loss and norm into slot k, correct predictions added, logits copied (logits_out may be NULL)
LG_LOCAL void lgt_file_step(const float* loss, const float* state, const float* logits, const float* lab, int N, int k,
                            float* losses, float* grad_norms, unsigned long long* correct, float* logits_out, hipStream_t s);
