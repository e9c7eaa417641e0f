// GraspPointCNN weights on gfx950 (see lg_cnn.h): the layer plan, the table of weight buffers, the fold kernels and the two
// loaders.  lg_cnn_upload (host tensors) and lg_cnn_upload_from_trainer (the trainer's device vectors) differ in where the
// PyTorch-layout tensors come from; everything after that -- plan, allocation, BatchNorm fold, Winograd transforms, fragment
// orders, load-time switches -- is build_weights() below, once.
#include "lg_cnn.h"
#include "lg_options.h"

#include <math.h>

#include <algorithm>
#include <vector>

int lg_cnn_plan(int n_blocks, const int32_t* filters, int attention_type, bool need_head, LgCnnPlan* p, std::string* err) {
    const int nb = n_blocks > 0 ? n_blocks : 3;
    int filt[4] = {64, 128, 256, 0};
    if (n_blocks > 0)
        for (int b = 0; b < 4; b++) filt[b] = filters[b];
    if (nb < 1 || nb > 4) { *err = "lg_cnn_load: 1..4 encoder blocks"; return LG_ERR_UNSUPPORTED; }
    *p = LgCnnPlan();
    p->n_layers = 2 * nb;
    int cin = 9, cinp = 10, wi = 32;
    size_t per = 0;
    for (int b = 0; b < nb; b++) {
        const int f = filt[b], fp = (f + 63) / 64 * 64;
        if (f < 16 || f > 512 || (f % 16) != 0) { *err = "lg_cnn_load: encoder filters must be multiples of 16 in [16, 512]"; return LG_ERR_UNSUPPORTED; }
        p->layers[2 * b] = {cin, f, cinp, fp, wi, false};
        p->layers[2 * b + 1] = {f, f, fp, fp, wi, true};
        per = std::max(per, (size_t)fp * wi * wi);
        cin = f; cinp = fp; wi /= 2;
    }
    const int F = filt[nb - 1];
    p->F = F; p->Fp = (F + 63) / 64 * 64; p->npix = wi * wi;
    p->act_per_patch = per;
    p->standard = nb == 3 && filt[0] == 64 && filt[1] == 128 && filt[2] == 256;
    p->hid = F / 16;
    const int dims[5] = {F, F, F / 2, F / 4, 1};
    std::copy(dims, dims + 5, p->dims);
    if (p->layers[0].coutp != 64 && p->layers[0].coutp != 128) { *err = "lg_cnn_load: first stage wider than 128 channels"; return LG_ERR_UNSUPPORTED; }
    for (int L = 1; L < p->n_layers; L++) {
        const RtLayer& l = p->layers[L];
        if (!wino_supported(l.cinp, l.coutp, l.wi, l.pool)) {
            *err = "lg_cnn_load: encoder_filters outside the reference's configurations ([32,64,128], [64,128,256], "
                   "[64,128,256,512], [128,256,512])";
            return LG_ERR_UNSUPPORTED;
        }
    }
    if (need_head && !lg_head_supported(F, p->npix)) { *err = "lg_cnn_forward: unsupported classifier size"; return LG_ERR_UNSUPPORTED; }
    if (attention_type < LG_ATT_SPATIAL || attention_type > LG_ATT_NONE) { *err = "lg_cnn_load: unknown attention_type"; return LG_ERR_INVALID; }
    return LG_OK;
}

// ================================================================== the fold, on the device
// One thread per output element group; IEEE double operations in a fixed association order, rounded once to float.  fp
// contraction is off in every body: the device would otherwise fuse a * b + c, and the weight bits are pinned by a reference
// that does not (tests/cnn_fold_ref.py).
namespace {

struct FoldConv {   // one encoder layer: PyTorch-layout tensors, padded geometry of the inference kernels
    const float *w, *b, *g, *be, *m, *v;
    int cin, cout, cinp, coutp, cinp4;
    float eps;
};

// scv = g / sqrt(v + eps) (eps: the float, promoted)
__device__ __forceinline__ double lg_fold_scale(const float* g, const float* v, int co, float eps) {
#pragma clang fp contract(off)
    return (double)g[co] / sqrt((double)v[co] + (double)eps);
}

// fold eval-mode BatchNorm2d: y = (conv + b - mean) * g / sqrt(var + eps) + beta; padded channels stay 0
// bconv [coutp] and wconv [tap][cinp][coutp] (wconv = nullptr: not for this layer); thread = (ci, co), co fastest
__global__ void lg_fold_direct_kernel(FoldConv a, float* __restrict__ bconv, float* __restrict__ wconv) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.cinp * a.coutp) return;
    const int co = t % a.coutp, ci = t / a.coutp;
    const bool real = co < a.cout;
    const double scv = real ? lg_fold_scale(a.g, a.v, co, a.eps) : 0.0;
    if (ci == 0) bconv[co] = real ? (float)(((double)a.b[co] - (double)a.m[co]) * scv + (double)a.be[co]) : 0.0f;
    if (!wconv) return;
    const float* src = a.w + ((size_t)co * a.cin + ci) * 9;
    for (int tap = 0; tap < 9; tap++)
        wconv[((size_t)tap * a.cinp + ci) * a.coutp + co] = real && ci < a.cin ? (float)((double)src[tap] * scv) : 0.0f;
}

// Winograd-domain weights U = G g G^T of the BN-folded kernel, in the order the kernels' A fragments are read:
// uwino (F(2x2,3x3), position 4i+j) [ci/4][co/16][q][lane][4] and uwino4 (F(4x4,3x3), position 6i+j)
// [ci/4][co/64][(co%64)/16][pg][lane][4], lane = (ci%4)*16 + co%16: both orders are
// (ci/4, co/16, lane) outside the position groups, so thread = (ci/4, co/16, lane) holds one (ci, co) pair and every float4 it
// stores lies next to its neighbour lane's -- one full 1 KB line per wave and position group.
// u2 = nullptr: layer 0 (no F(2x2) weights); its F(4x4) weights have cinp4 = 12 input planes.
__global__ void lg_fold_wino_kernel(FoldConv a, float* __restrict__ u2, float* __restrict__ u4) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nb16 = a.coutp / 16;
    if (t >= (a.cinp4 / 4) * nb16 * 64) return;
    const int lane = t % 64, b16 = (t / 64) % nb16, k = t / (64 * nb16);
    const int ci = 4 * k + lane / 16, co = 16 * b16 + lane % 16;
    const bool real = ci < a.cin && co < a.cout;
    double g[3][3];
    if (real) {
        const double scv = lg_fold_scale(a.g, a.v, co, a.eps);
        const float* src = a.w + ((size_t)co * a.cin + ci) * 9;
        for (int tap = 0; tap < 9; tap++) g[tap / 3][tap % 3] = (double)src[tap] * scv;
    }
    if (u2 && ci < a.cinp) {
        float4* u = (float4*)(u2 + ((((size_t)k * nb16 + b16) * 4) * 64 + lane) * 4);
        if (real) {
            double gg[4][3];
            for (int j = 0; j < 3; j++) {
                gg[0][j] = g[0][j];
                gg[1][j] = 0.5 * (g[0][j] + g[1][j] + g[2][j]);
                gg[2][j] = 0.5 * (g[0][j] - g[1][j] + g[2][j]);
                gg[3][j] = g[2][j];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                u[64 * i] = make_float4((float)gg[i][0], (float)(0.5 * (gg[i][0] + gg[i][1] + gg[i][2])),
                                        (float)(0.5 * (gg[i][0] - gg[i][1] + gg[i][2])), (float)gg[i][2]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) u[64 * i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    {
        constexpr double G4[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                     {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
        // ((k * ncb + co/64) * 4 + (co%64)/16) = k * nb16 + b16
        float4* u = (float4*)(u4 + ((((size_t)k * nb16 + b16) * 9) * 64 + lane) * 4);
        if (real) {
            double gg[6][3];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) gg[i][j] = G4[i][0] * g[0][j] + G4[i][1] * g[1][j] + G4[i][2] * g[2][j];
            float o[36];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) o[6 * i + j] = (float)(gg[i][0] * G4[j][0] + gg[i][1] * G4[j][1] + gg[i][2] * G4[j][2]);
#pragma unroll
            for (int pg = 0; pg < 9; pg++) u[64 * pg] = make_float4(o[4 * pg], o[4 * pg + 1], o[4 * pg + 2], o[4 * pg + 3]);
        } else {
#pragma unroll
            for (int pg = 0; pg < 9; pg++) u[64 * pg] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// classifier layer: fcw [in][out] (transposed) and fcb [out], BatchNorm1d folded where g is given; thread = (i, o), o fastest
__global__ void lg_fold_fc_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ g,
                                  const float* __restrict__ be, const float* __restrict__ m, const float* __restrict__ v, float eps,
                                  int fin, int fout, float* __restrict__ wt, float* __restrict__ bt) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= fin * fout) return;
    const int o = t % fout, i = t / fout;
    double sc = 1.0, sh = 0.0;
    if (g) {
        sc = (double)g[o] / sqrt((double)v[o] + (double)eps);
        sh = (double)be[o] - (double)m[o] * sc;
    }
    if (i == 0) bt[o] = (float)((double)b[o] * sc + sh);
    wt[(size_t)i * fout + o] = (float)((double)w[(size_t)o * fin + i] * sc);
}

// ================================================================== the weight buffers of a model
struct WeightBuf { float** slot; size_t n; int which, layer; };   // pointer slot in LgCnn, floats, LG_CNNW_* code, layer
constexpr int LG_MAX_WEIGHT_BUFS = 8 * 4 + 5 + 4 * 2 + 1;
constexpr size_t LG_ZERO_FLOATS = 4096;   // zeroed plane: padding channel of layer 0, unused staging slots

// every weight buffer of the plan and attention type that *c holds; -> how many
int weight_buffers(LgCnn* c, WeightBuf* out) {
    int n = 0;
    for (int L = 0; L < c->n_layers; L++) {
        const RtLayer& l = c->layers[L];
        out[n++] = {&c->bconv[L], (size_t)l.coutp, LG_CNNW_BCONV, L};
        // direct implicit-GEMM weights: layer 0; A/B path of the standard model
        if (L == 0 || c->standard) out[n++] = {&c->wconv[L], (size_t)9 * l.cinp * l.coutp, LG_CNNW_WCONV, L};
        if (L >= 1) out[n++] = {&c->uwino[L], (size_t)16 * l.cinp * l.coutp, LG_CNNW_UWINO, L};
        out[n++] = {&c->uwino4[L], (size_t)36 * (L == 0 ? 12 : l.cinp) * l.coutp, LG_CNNW_UWINO4, L};   // layer 0: 9 feature planes + 3 zero planes
    }
    const size_t F = c->F, hid = c->hid;
    if (c->att_type == LG_ATT_SPATIAL || c->att_type == LG_ATT_HYBRID) out[n++] = {&c->att_w, F, LG_CNNW_ATT_W, 0};
    if (c->att_type == LG_ATT_CHANNEL || c->att_type == LG_ATT_HYBRID) {
        out[n++] = {&c->ca_w1, hid * F, LG_CNNW_CA_W1, 0};
        out[n++] = {&c->ca_b1, hid, LG_CNNW_CA_B1, 0};
        out[n++] = {&c->ca_w2, F * hid, LG_CNNW_CA_W2, 0};
        out[n++] = {&c->ca_b2, F, LG_CNNW_CA_B2, 0};
    }
    for (int L = 0; L < 4; L++) {
        out[n++] = {&c->fcw[L], (size_t)c->dims[L] * c->dims[L + 1], LG_CNNW_FCW, L};
        out[n++] = {&c->fcb[L], (size_t)c->dims[L + 1], LG_CNNW_FCB, L};
    }
    out[n++] = {&c->zeros, LG_ZERO_FLOATS, LG_CNNW_ZEROS, 0};
    return n;
}

int load_failed(LgCnn* c, std::string* err) {
    (void)hipGetLastError();
    lg_cnn_free(c);   // half-written weights are no model
    *err = "lg_cnn_load: device allocation/copy failed";
    return LG_ERR_HIP;
}

// The weights of plan p / attention type v->att from the PyTorch-layout tensors of *v, on stream s; synchronises s.  Same
// geometry as the loaded model: its buffers are rewritten where they are; else the model is freed and allocated anew.
int build_weights(LgCnn* c, const LgCnnPlan& p, const LgTrainView* v, hipStream_t s, std::string* err) {
    const float eps = v->bn_eps > 0.f ? v->bn_eps : 1e-5f;
    WeightBuf wb[LG_MAX_WEIGHT_BUFS];
    bool same = c->loaded && c->n_layers == p.n_layers && c->att_type == v->att;
    for (int L = 0; L < p.n_layers && same; L++) {
        const RtLayer &x = c->layers[L], &y = p.layers[L];
        same = x.cin == y.cin && x.cout == y.cout && x.cinp == y.cinp && x.coutp == y.coutp && x.wi == y.wi && x.pool == y.pool;
    }
    if (same)
        for (int i = 0, n = weight_buffers(c, wb); i < n && same; i++) same = *wb[i].slot != nullptr;
    if (!same) {
        lg_cnn_free(c);
        static_cast<LgCnnPlan&>(*c) = p;
        c->att_type = v->att;
        c->att_b = 0.f;
        for (int i = 0, n = weight_buffers(c, wb); i < n; i++) {
            if (hipMalloc((void**)wb[i].slot, wb[i].n * sizeof(float)) != hipSuccess) return load_failed(c, err);
            c->weight_allocs++;
        }
        if (hipMemsetAsync(c->zeros, 0, LG_ZERO_FLOATS * sizeof(float), s) != hipSuccess) return load_failed(c, err);
    }
    c->loaded = false;   // until every launch below is in the stream

    // ---- fold + transforms
    for (int L = 0; L < p.n_layers; L++) {
        const RtLayer& l = p.layers[L];
        FoldConv a = {v->P + v->conv_w[L], v->P + v->conv_b[L], v->P + v->bn_g[L], v->P + v->bn_b[L], v->B + v->bn_m[L], v->B + v->bn_v[L],
                      l.cin, l.cout, l.cinp, l.coutp, L == 0 ? 12 : l.cinp, eps};
        hipLaunchKernelGGL(lg_fold_direct_kernel, dim3((unsigned)((l.cinp * l.coutp + 255) / 256)), dim3(256), 0, s, a, c->bconv[L],
                           c->wconv[L]);
        hipLaunchKernelGGL(lg_fold_wino_kernel, dim3((unsigned)((a.cinp4 / 4 * (l.coutp / 16) * 64 + 255) / 256)), dim3(256), 0, s, a,
                           c->uwino[L], c->uwino4[L]);
    }
    for (int L = 0; L < 4; L++) {
        const bool bn = L < 3;
        hipLaunchKernelGGL(lg_fold_fc_kernel, dim3((unsigned)((p.dims[L] * p.dims[L + 1] + 255) / 256)), dim3(256), 0, s, v->P + v->fc_w[L],
                           v->P + v->fc_b[L], bn ? v->P + v->fbn_g[L] : nullptr, bn ? v->P + v->fbn_b[L] : nullptr,
                           bn ? v->B + v->fbn_m[L] : nullptr, bn ? v->B + v->fbn_v[L] : nullptr, eps, p.dims[L], p.dims[L + 1], c->fcw[L],
                           c->fcb[L]);
    }
    bool ok = hipGetLastError() == hipSuccess;
    auto D2D = [&](float* dst, size_t off, size_t n) {
        if (dst && ok && hipMemcpyAsync(dst, v->P + off, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) ok = false;
    };
    const size_t F = p.F, hid = p.hid;
    D2D(c->att_w, v->att_w, F);
    D2D(c->ca_w1, v->ca_w1, hid * F); D2D(c->ca_b1, v->ca_b1, hid); D2D(c->ca_w2, v->ca_w2, F * hid); D2D(c->ca_b2, v->ca_b2, F);
    // lg_head_kernel takes the spatial attention's bias by value: the one scalar that comes back to the host
    float att_b = 0.f;
    if (c->att_w && ok && hipMemcpyAsync(&att_b, v->P + v->att_b, sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) ok = false;
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return load_failed(c, err);
    c->att_b = att_b;
    // A/B and test switches of the standard encoder, read when a model is loaded (not on the per-call path):
    // LG_CNN_DIRECT=1 direct implicit GEMM for every layer; LG_CNN_WINO_MASK=<bits> bit L = layer L on Winograd
    // LG_CNN_F23=1 the F(2x2,3x3) Winograd kernels instead of F(4x4,3x3)
    const LgCnnOptions o = lg_cnn_options_from_env();
    c->use_f23 = o.f23;
    c->wino_mask = o.wino_mask;
    c->loaded = true;
    return LG_OK;
}

}  // namespace

void lg_cnn_free(LgCnn* c) {
    auto F = [](float*& p) { if (p) hipFree(p); p = nullptr; };
    WeightBuf wb[LG_MAX_WEIGHT_BUFS];
    for (int i = 0, n = weight_buffers(c, wb); i < n; i++) F(*wb[i].slot);
    for (int i = 0; i < 8; i++) F(c->act[i]);
    F(c->in_halo); F(c->kpart);
    if (c->kflag) { hipFree(c->kflag); c->kflag = nullptr; }
    if (c->kerr_host) { hipHostFree(c->kerr_host); c->kerr_host = nullptr; c->kerr_dev = nullptr; }
    c->capN = 0;
    c->loaded = false;
}

bool lg_cnn_weight_buffer(const LgCnn* c, int which, int layer, const float** p, size_t* n) {
    *p = nullptr; *n = 0;
    if (!c->loaded) return false;
    WeightBuf wb[LG_MAX_WEIGHT_BUFS];
    const int cnt = weight_buffers(const_cast<LgCnn*>(c), wb);   // (the table's slots are writable; they are only read here)
    for (int i = 0; i < cnt; i++)
        if (wb[i].which == which && (which >= LG_CNNW_ATT_W || wb[i].layer == layer) && *wb[i].slot) {   // one per model: `layer` is ignored
            *p = *wb[i].slot; *n = wb[i].n;
            return true;
        }
    return false;
}

int lg_cnn_upload_from_trainer(LgCnn* c, const LgTrainView* v, hipStream_t s, std::string* err) {
    // nothing of *c is touched before the model is known to run
    LgCnnPlan p;
    const int rc = lg_cnn_plan(v->n_blocks, v->filters, v->att, true, &p, err);
    if (rc) return rc;
    if (!v->P || !v->B || v->F != p.F) { *err = "lg_cnn_load: missing encoder tensor"; return LG_ERR_INVALID; }
    return build_weights(c, p, v, s, err);
}

int lg_cnn_upload(LgCnn* c, const lg_cnn_weights* w, std::string* err) {
    lg_cnn_free(c);   // a load starts from scratch: a refused one leaves no model
    LgCnnPlan p;
    const int rc = lg_cnn_plan(w->n_blocks, w->filters, w->attention_type, false, &p, err);
    if (rc == LG_ERR_UNSUPPORTED) return rc;
    // ---- the caller's host tensors into one flat vector, laid out as an LgTrainView (P and B share it)
    std::vector<float> flat;
    bool missing = false;
    auto put = [&](const float* src, size_t n) {
        const size_t off = flat.size();
        if (src) flat.insert(flat.end(), src, src + n); else missing = true;
        return off;
    };
    LgTrainView v;
    v.n_blocks = p.n_layers / 2; v.att = w->attention_type; v.F = p.F; v.hid = p.hid;
    v.bn_eps = w->bn_eps;
    for (int L = 0; L < p.n_layers; L++) {
        const RtLayer& l = p.layers[L];
        v.conv_w[L] = put(w->conv_w[L], (size_t)l.cout * l.cin * 9); v.conv_b[L] = put(w->conv_b[L], l.cout);
        v.bn_g[L] = put(w->bn_g[L], l.cout); v.bn_b[L] = put(w->bn_b[L], l.cout);
        v.bn_m[L] = put(w->bn_m[L], l.cout); v.bn_v[L] = put(w->bn_v[L], l.cout);
    }
    if (missing) { *err = "lg_cnn_load: missing encoder tensor"; return LG_ERR_INVALID; }
    if (rc) return rc;   // the plan's last check, the attention type: after the encoder tensors, as ever
    const size_t F = p.F, hid = p.hid;
    if (v.att == LG_ATT_SPATIAL || v.att == LG_ATT_HYBRID) {
        v.att_w = put(w->att_w, F); v.att_b = put(w->att_b, 1);
        if (missing) { *err = "lg_cnn_load: missing spatial attention tensor"; return LG_ERR_INVALID; }
    }
    if (v.att == LG_ATT_CHANNEL || v.att == LG_ATT_HYBRID) {
        v.ca_w1 = put(w->ca_w1, hid * F); v.ca_b1 = put(w->ca_b1, hid); v.ca_w2 = put(w->ca_w2, F * hid); v.ca_b2 = put(w->ca_b2, F);
        if (missing) { *err = "lg_cnn_load: missing channel attention tensor"; return LG_ERR_INVALID; }
    }
    for (int L = 0; L < 4; L++) {
        const size_t fin = p.dims[L], fout = p.dims[L + 1];
        v.fc_w[L] = put(w->fc_w[L], fin * fout); v.fc_b[L] = put(w->fc_b[L], fout);
        if (missing) { *err = "lg_cnn_load: missing classifier tensor"; return LG_ERR_INVALID; }
        if (L == 3) break;
        v.fbn_g[L] = put(w->fbn_g[L], fout); v.fbn_b[L] = put(w->fbn_b[L], fout);
        v.fbn_m[L] = put(w->fbn_m[L], fout); v.fbn_v[L] = put(w->fbn_v[L], fout);
        if (missing) { *err = "lg_cnn_load: missing classifier BN tensor"; return LG_ERR_INVALID; }
    }
    float* staged = nullptr;
    if (hipMalloc((void**)&staged, flat.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(staged, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        if (staged) hipFree(staged);
        return load_failed(c, err);
    }
    v.P = v.B = staged;
    const int rb = build_weights(c, p, &v, nullptr, err);   // the legacy default stream, synchronised
    hipFree(staged);
    return rb;
}
