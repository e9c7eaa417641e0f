// GraspPointCNN training step on gfx950: forward in train mode (batch-statistics BatchNorm, Dropout2d / Dropout with
// explicit keep masks), BCEWithLogits(pos_weight) loss, backward, global-norm gradient clipping and Adam with L2 weight
// decay -- one call = one iteration of the inner loop of scripts/train_model.py:247-265 on the model of
// scripts/utils/ml_grasp_optimizer/model.py:5-128 (every attention type -- 'spatial' is the script's default --,
// any encoder_filters of the reference's sweep).
//
// This file is the host side: the handle, the lg_train_* entries and enqueue_step, the recipe of a step written as calls of
// the launchers in lg_train.h.  The kernels stand with their launchers in lg_train_conv.hip (the MFMA convolutions),
// lg_train_layers.hip (BatchNorm, pooling, attention, classifier) and lg_train_optim.hip (loss, optimizer, masks, the
// device epoch's gather and filing).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/leafgrasp.h"
#include "lg_cnn.h"
#include "lg_options.h"
#include "lg_train.h"

struct TrainLayer {
    int ci = 0, co = 0, wi = 0;
    bool pool = false;
    size_t w = 0, b = 0, g = 0, be = 0;   // offsets into the flat parameter vector
    size_t rm = 0, rv = 0;                // offsets into the flat buffer vector (running mean / var)
    size_t st = 0;                        // offset into the saved mean / rstd vector
    float *x = nullptr, *out = nullptr;   // conv output (pre-BN), layer output (post BN/ReLU[/pool/dropout])
    float *wpf = nullptr, *wpd = nullptr;
    size_t mask = 0;                      // offset of the block's Dropout2d mask inside one sample's mask row (pool layers)
};
struct TrainFc { int in = 0, out = 0; size_t w = 0, b = 0, g = 0, be = 0, rm = 0, rv = 0, st = 0, mask = 0; float *u = nullptr, *y = nullptr; };

struct lg_trainer {
    int device = 0, n_blocks = 3, att = LG_ATT_SPATIAL, capN = 0, F = 256, P = 16;
    int filters[4] = {64, 128, 256, 0};
    std::vector<TrainLayer> layers;
    TrainFc fc[4];
    size_t att_w = 0, att_b = 0, ca_w1 = 0, ca_b1 = 0, ca_w2 = 0, ca_b2 = 0;
    int hid = 0;                                  // channel attention bottleneck: F / 16
    float *ca_m = nullptr, *ca_z1 = nullptr, *ca_r = nullptr, *ca_z2 = nullptr, *ca_ca = nullptr, *gap2 = nullptr;
    float *ca_dgs = nullptr, *ca_dz2 = nullptr, *ca_dr = nullptr, *ca_dz1 = nullptr, *ca_dm = nullptr, *ca_a1 = nullptr;
    size_t n_params = 0, n_buffers = 0, n_stats = 0, mask_row = 0;
    float drop2d_p = 0.3f, drop_p[3] = {0.5f, 0.5f, 0.4f};
    float *P_ = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *B = nullptr, *mean = nullptr, *rstd = nullptr;
    float *xin = nullptr, *labels = nullptr, *masks = nullptr;
    float *dA[2] = {nullptr, nullptr}, *dX[2] = {nullptr, nullptr}, *partial = nullptr, *bn_part = nullptr;
    size_t partial_floats = 0;
    float *att_a = nullptr, *gap = nullptr, *att_part = nullptr, *dfc[2] = {nullptr, nullptr}, *logits = nullptr, *dz = nullptr;
    float *loss = nullptr, *state = nullptr, *norm_part = nullptr;
    AdamHp* hp = nullptr;
    hipStream_t stream = nullptr, stream_w = nullptr;   // main chain; backward-weights branch
    hipEvent_t ev_dx[8] = {}, ev_wg[8] = {};
    uint64_t* seed_dev = nullptr;
    bool side_stream = false;                    // backward-weights on stream_w (LG_TRAIN_STREAMS=2); default: in line
    LgtConvCut conv_cut;                         // convolution shape thresholds (lgt_conv)
    bool use_graph = false;                      // LG_TRAIN_GRAPH=1: replay the step as a captured graph (measured: no gain)
    std::map<uint64_t, hipGraphExec_t> graphs;   // key: N, masks drawn on the device, optimizer applied
    int64_t steps = 0;
    void* epoch_dev = nullptr;                   // lg_train_epoch: counter, loss and norm slots, indices; grown on demand
    size_t epoch_bytes = 0;
    std::string err;
    std::vector<void*> allocs;
};

namespace {

#define TR_HIP(call)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            tr->err = std::string(#call) + ": " + hipGetErrorString(e_);                                 \
            return LG_ERR_HIP;                                                                           \
        }                                                                                                \
    } while (0)

int dalloc(lg_trainer* tr, float** p, size_t floats) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(floats, 1) * sizeof(float)) != hipSuccess) {
        tr->err = "hipMalloc failed";
        return LG_ERR_NOMEM;
    }
    tr->allocs.push_back(q);
    *p = (float*)q;
    return LG_OK;
}

// a call's hyper-parameters to the device, in stream order in front of the step that reads them
int upload_hp(lg_trainer* tr, const lg_train_hparams* hp) {
    hipStream_t s = tr->stream;
    const AdamHp h = {hp->lr, hp->beta1, hp->beta2, hp->eps, hp->weight_decay, hp->max_grad_norm, hp->pos_weight, 0.0f};
    TR_HIP(hipMemcpyAsync(tr->hp, &h, sizeof(h), hipMemcpyHostToDevice, s));
    return LG_OK;
}

// conv biases: exact zero gradient (see DESIGN), no kernel writes them.  In front of every enqueue_step and outside the captured
// graph, like the copies of a step's inputs.
// OBSERVED, not understood: captured with the step (the graph's only memset node), G was zero after the graph's first
// launch, and after every later launch exactly the entries that only this memset writes held ~1e18
// (tests/test_gpu_train_modes.py, profiles/NOTES_train_tests.md).  The cause inside the runtime is unknown; this says
// nothing about memset nodes in general.
int zero_grads(lg_trainer* tr) {
    hipStream_t s = tr->stream;
    TR_HIP(hipMemsetAsync(tr->G, 0, tr->n_params * 4, s));
    return LG_OK;
}

}  // namespace

extern "C" {

int lg_train_create(int device, int n_blocks, const int32_t* filters, int attention_type, int max_batch, lg_trainer** out) {
    if (!out) return LG_ERR_INVALID;
    *out = nullptr;
    if (!filters || n_blocks < 1 || n_blocks > 4 || max_batch < 2 || max_batch > 8192) return LG_ERR_INVALID;
    if (attention_type < LG_ATT_SPATIAL || attention_type > LG_ATT_NONE) return LG_ERR_UNSUPPORTED;
    for (int b = 0; b < n_blocks; b++)
        if (filters[b] < 32 || filters[b] % 32 != 0 || filters[b] > kLgtMaxChannels) return LG_ERR_INVALID;
    if (filters[n_blocks - 1] % 4 != 0) return LG_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return LG_ERR_HIP;
    lg_trainer* tr = new (std::nothrow) lg_trainer;
    if (!tr) return LG_ERR_NOMEM;
    tr->device = device;
    tr->n_blocks = n_blocks;
    tr->att = attention_type;
    tr->capN = max_batch;
    hipSetDevice(device);

    // parameter order = model.parameters() of the reference module (model.py:12-85)
    size_t po = 0, bo = 0, so = 0, mo = 0;
    int c = 9, wi = 32;
    for (int b = 0; b < n_blocks; b++) {
        tr->filters[b] = filters[b];
        for (int k = 0; k < 2; k++) {
            TrainLayer L;
            L.ci = k == 0 ? c : filters[b];
            L.co = filters[b];
            L.wi = wi;
            L.pool = k == 1;
            L.w = po; po += (size_t)L.co * L.ci * 9;
            L.b = po; po += L.co;
            L.g = po; po += L.co;
            L.be = po; po += L.co;
            L.rm = bo; bo += L.co;
            L.rv = bo; bo += L.co;
            L.st = so; so += L.co;
            if (L.pool) { L.mask = mo; mo += L.co; }
            tr->layers.push_back(L);
        }
        c = filters[b];
        wi /= 2;
    }
    const int F = c;
    tr->F = F;
    tr->P = wi * wi;
    if (filters[n_blocks - 1] % 16 != 0 && (attention_type == LG_ATT_CHANNEL || attention_type == LG_ATT_HYBRID)) {
        delete tr;
        return LG_ERR_INVALID;
    }
    if (attention_type == LG_ATT_SPATIAL || attention_type == LG_ATT_HYBRID) {   // attention.0 / spatial_attention.0
        tr->att_w = po; po += F;
        tr->att_b = po; po += 1;
    }
    if (attention_type == LG_ATT_CHANNEL || attention_type == LG_ATT_HYBRID) {   // attention.{1,3} / channel_attention.{1,3}
        tr->hid = F / 16;
        tr->ca_w1 = po; po += (size_t)tr->hid * F;
        tr->ca_b1 = po; po += tr->hid;
        tr->ca_w2 = po; po += (size_t)F * tr->hid;
        tr->ca_b2 = po; po += F;
    }
    const int fin[4] = {F, F, F / 2, F / 4}, fout[4] = {F, F / 2, F / 4, 1};
    for (int k = 0; k < 4; k++) {
        TrainFc& f = tr->fc[k];
        f.in = fin[k];
        f.out = fout[k];
        f.w = po; po += (size_t)f.in * f.out;
        f.b = po; po += f.out;
        if (k < 3) {
            f.g = po; po += f.out;
            f.be = po; po += f.out;
            f.rm = bo; bo += f.out;
            f.rv = bo; bo += f.out;
            f.st = so; so += f.out;
            f.mask = mo; mo += f.out;
        }
    }
    tr->n_params = po;
    tr->n_buffers = bo;
    tr->n_stats = so;
    tr->mask_row = mo;

    const size_t N = (size_t)max_batch;
    int rc = LG_OK;
    auto A = [&](float** p, size_t n) { if (rc == LG_OK) rc = dalloc(tr, p, n); };
    A(&tr->P_, po); A(&tr->G, po); A(&tr->M, po); A(&tr->V, po); A(&tr->B, bo); A(&tr->mean, so); A(&tr->rstd, so);
    A(&tr->xin, N * 9 * 1024); A(&tr->labels, N); A(&tr->masks, N * mo);
    size_t max_act = 0;
    for (auto& L : tr->layers) {
        const size_t full = N * L.co * L.wi * L.wi;
        A(&L.x, full);
        A(&L.out, L.pool ? full / 4 : full);
        A(&L.wpf, (size_t)9 * L.ci * L.co);
        A(&L.wpd, (size_t)9 * L.ci * L.co);
        max_act = std::max(max_act, std::max(full, N * L.ci * L.wi * L.wi));
        tr->partial_floats = std::max(tr->partial_floats, lgt_wgrad_partial_floats(L.wi, max_batch, L.ci, L.co));
    }
    A(&tr->dA[0], max_act); A(&tr->dA[1], max_act); A(&tr->dX[0], max_act); A(&tr->dX[1], max_act);
    A(&tr->partial, tr->partial_floats); A(&tr->bn_part, lgt_bn_part_floats());
    A(&tr->att_a, N * tr->P); A(&tr->gap, N * F); A(&tr->att_part, lgt_att_part_floats(max_batch, F));
    if (tr->hid) {
        A(&tr->ca_m, N * F); A(&tr->ca_z1, N * tr->hid); A(&tr->ca_r, N * tr->hid); A(&tr->ca_z2, N * F); A(&tr->ca_ca, N * F);
        A(&tr->gap2, N * F); A(&tr->ca_dgs, N * F); A(&tr->ca_dz2, N * F); A(&tr->ca_dr, N * tr->hid); A(&tr->ca_dz1, N * tr->hid);
        A(&tr->ca_dm, N * F); A(&tr->ca_a1, N * tr->P);
    }
    A(&tr->dfc[0], N * F); A(&tr->dfc[1], N * F); A(&tr->logits, N); A(&tr->dz, N);
    for (int k = 0; k < 4; k++) { A(&tr->fc[k].u, N * tr->fc[k].out); if (k < 3) A(&tr->fc[k].y, N * tr->fc[k].out); }
    A(&tr->loss, 4); A(&tr->state, 4); A(&tr->norm_part, lgt_norm_part_floats());
    float *hp = nullptr, *sd = nullptr;
    A(&hp, sizeof(AdamHp) / sizeof(float));
    tr->hp = (AdamHp*)hp;
    A(&sd, 2);
    tr->seed_dev = (uint64_t*)sd;
    const LgTrainOptions o = lg_train_options_from_env();
    tr->use_graph = o.graph;
    tr->conv_cut = {o.conv_small_below, o.conv_split_below};
    if (rc == LG_OK && hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking) != hipSuccess) rc = LG_ERR_HIP;
    if (rc == LG_OK && hipStreamCreateWithFlags(&tr->stream_w, hipStreamNonBlocking) != hipSuccess) rc = LG_ERR_HIP;
    for (int k = 0; k < 8 && rc == LG_OK; k++)
        if (hipEventCreateWithFlags(&tr->ev_dx[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&tr->ev_wg[k], hipEventDisableTiming) != hipSuccess) rc = LG_ERR_HIP;
    if (rc != LG_OK) {
        for (void* q : tr->allocs) hipFree(q);
        for (int k = 0; k < 8; k++) {
            if (tr->ev_dx[k]) hipEventDestroy(tr->ev_dx[k]);
            if (tr->ev_wg[k]) hipEventDestroy(tr->ev_wg[k]);
        }
        if (tr->stream) hipStreamDestroy(tr->stream);
        if (tr->stream_w) hipStreamDestroy(tr->stream_w);
        delete tr;
        return rc;
    }
    hipMemset(tr->P_, 0, po * 4); hipMemset(tr->G, 0, po * 4); hipMemset(tr->M, 0, po * 4); hipMemset(tr->V, 0, po * 4);
    hipMemset(tr->B, 0, bo * 4); hipMemset(tr->state, 0, 16); hipMemset(tr->loss, 0, 16);
    hipDeviceSynchronize();
    // Backward-weights runs in line on the one stream by default.  On a second stream (LG_TRAIN_STREAMS=2: stream_w, dX double
    // buffered, event fences) it overlaps the BatchNorm-backward / backward-data chain and gains 2-5 % at batches 64..1024 --
    // but each of the ~12 stream hops of a step costs ~15 us (0.65 vs 0.67 ms at batch 16), and how ROCm maps a process's
    // streams to its few hardware queues depends on how many streams exist when these two are created: for 2 of 9 probed
    // counts (tests/tools/streams_probe.py) the two-stream step was 2.2-2.5x slower.
    tr->side_stream = o.streams == 2;
    *out = tr;
    return LG_OK;
}

int lg_train_destroy(lg_trainer* tr) {
    if (!tr) return LG_ERR_INVALID;
    hipSetDevice(tr->device);
    hipDeviceSynchronize();
    for (auto& kv : tr->graphs) hipGraphExecDestroy(kv.second);
    if (tr->stream) hipStreamDestroy(tr->stream);
    if (tr->stream_w) hipStreamDestroy(tr->stream_w);
    for (int k = 0; k < 8; k++) {
        if (tr->ev_dx[k]) hipEventDestroy(tr->ev_dx[k]);
        if (tr->ev_wg[k]) hipEventDestroy(tr->ev_wg[k]);
    }
    for (void* q : tr->allocs) hipFree(q);
    if (tr->epoch_dev) hipFree(tr->epoch_dev);
    delete tr;
    return LG_OK;
}

const char* lg_train_last_error(lg_trainer* tr) { return tr ? tr->err.c_str() : "null trainer"; }

int lg_train_sizes(lg_trainer* tr, int64_t* n_params, int64_t* n_buffers, int64_t* mask_row) {
    if (!tr) return LG_ERR_INVALID;
    if (n_params) *n_params = (int64_t)tr->n_params;
    if (n_buffers) *n_buffers = (int64_t)tr->n_buffers;
    if (mask_row) *mask_row = (int64_t)tr->mask_row;
    return LG_OK;
}

int lg_train_set_state(lg_trainer* tr, const float* params, const float* buffers, const float* exp_avg,
                       const float* exp_avg_sq, int64_t step) {
    if (!tr || !params || !buffers || step < 0) return LG_ERR_INVALID;
    hipSetDevice(tr->device);
    TR_HIP(hipStreamSynchronize(tr->stream));
    TR_HIP(hipMemcpy(tr->P_, params, tr->n_params * 4, hipMemcpyHostToDevice));
    TR_HIP(hipMemcpy(tr->B, buffers, tr->n_buffers * 4, hipMemcpyHostToDevice));
    if (exp_avg) TR_HIP(hipMemcpy(tr->M, exp_avg, tr->n_params * 4, hipMemcpyHostToDevice));
    else TR_HIP(hipMemset(tr->M, 0, tr->n_params * 4));
    if (exp_avg_sq) TR_HIP(hipMemcpy(tr->V, exp_avg_sq, tr->n_params * 4, hipMemcpyHostToDevice));
    else TR_HIP(hipMemset(tr->V, 0, tr->n_params * 4));
    const float st[4] = {(float)step, 0.f, 0.f, 0.f};
    TR_HIP(hipMemcpy(tr->state, st, 16, hipMemcpyHostToDevice));
    tr->steps = step;
    return LG_OK;
}

int lg_train_get_state(lg_trainer* tr, float* params, float* buffers, float* exp_avg, float* exp_avg_sq, float* grads,
                       int64_t* step) {
    if (!tr) return LG_ERR_INVALID;
    hipSetDevice(tr->device);
    TR_HIP(hipStreamSynchronize(tr->stream));
    if (params) TR_HIP(hipMemcpy(params, tr->P_, tr->n_params * 4, hipMemcpyDeviceToHost));
    if (buffers) TR_HIP(hipMemcpy(buffers, tr->B, tr->n_buffers * 4, hipMemcpyDeviceToHost));
    if (exp_avg) TR_HIP(hipMemcpy(exp_avg, tr->M, tr->n_params * 4, hipMemcpyDeviceToHost));
    if (exp_avg_sq) TR_HIP(hipMemcpy(exp_avg_sq, tr->V, tr->n_params * 4, hipMemcpyDeviceToHost));
    if (grads) TR_HIP(hipMemcpy(grads, tr->G, tr->n_params * 4, hipMemcpyDeviceToHost));
    if (step) *step = tr->steps;
    return LG_OK;
}

// Everything of a step whose launch parameters depend only on (N, draw_masks, apply_update): captured into a graph.
static int enqueue_step(lg_trainer* tr, int N, bool draw_masks, int apply_update) {
    hipStream_t s = tr->stream;
    const int F = tr->F, P = tr->P;
    const float eps = 1e-5f, mom = 0.1f;
    float *const W = tr->P_, *const G = tr->G;   // parameters and their gradients, same offsets
    if (draw_masks) {
        MaskTable mt = {};
        for (auto& L : tr->layers)
            if (L.pool) { mt.end[mt.n] = (size_t)N * (L.mask + L.co); mt.p[mt.n++] = tr->drop2d_p; }
        for (int k = 0; k < 3; k++) { mt.end[mt.n] = (size_t)N * (tr->fc[k].mask + tr->fc[k].out); mt.p[mt.n++] = tr->drop_p[k]; }
        lgt_draw_masks(tr->masks, mt, tr->seed_dev, tr->state, s);
    }
    {
        PackTable pt = {};
        unsigned end = 0;
        for (auto& L : tr->layers) {
            const int k = pt.n++;
            pt.w[k] = W + L.w; pt.wpf[k] = L.wpf; pt.wpd[k] = L.wpd; pt.ci[k] = L.ci; pt.co[k] = L.co;
            end += (unsigned)(9 * L.ci * L.co);
            pt.end[k] = end;
        }
        lgt_pack(pt, s);
    }

    // ---------------- forward
    const float* a = tr->xin;
    for (auto& L : tr->layers) {
        lgt_conv(tr->conv_cut, L.wi, a, L.wpf, W + L.b, L.x, N, L.ci, L.co, s);
        lgt_bn2d_fwd(L.x, W + L.g, W + L.be, L.pool ? tr->masks + (size_t)N * L.mask : nullptr, tr->bn_part, tr->mean + L.st,
                     tr->rstd + L.st, tr->B + L.rm, tr->B + L.rv, L.out, N, L.co, L.wi, eps, mom, s);
        a = L.out;
    }
    const int spatial = tr->att == LG_ATT_SPATIAL || tr->att == LG_ATT_HYBRID;
    const int hid = tr->hid;
    const size_t nh = (size_t)N * hid, nf = (size_t)N * F;
    lgt_att_fwd(a, W + tr->att_w, W + tr->att_b, spatial, N, F, P, tr->att_a, tr->gap, s);
    const float* pooled = tr->gap;
    const float* ca_in = tr->gap;   // 'channel': the plain mean is the pooled feature itself
    if (hid) {
        if (spatial) {              // 'hybrid': the channel branch pools the unattended map
            lgt_att_fwd(a, W + tr->att_w, W + tr->att_b, 0, N, F, P, tr->ca_a1, tr->ca_m, s);
            ca_in = tr->ca_m;
        }
        lgt_fc_fwd(ca_in, W + tr->ca_w1, W + tr->ca_b1, tr->ca_z1, N, F, hid, s);
        lgt_relu_fwd(tr->ca_z1, tr->ca_r, nh, s);
        lgt_fc_fwd(tr->ca_r, W + tr->ca_w2, W + tr->ca_b2, tr->ca_z2, N, hid, F, s);
        lgt_catt_gate_fwd(tr->ca_z2, tr->gap, tr->ca_ca, tr->gap2, nf, s);
        pooled = tr->gap2;
    }
    const float* fin = pooled;
    for (int k = 0; k < 4; k++) {
        TrainFc& f = tr->fc[k];
        lgt_fc_fwd(fin, W + f.w, W + f.b, k < 3 ? f.u : tr->logits, N, f.in, f.out, s);
        if (k < 3) {
            lgt_bn1d_fwd(f.u, W + f.g, W + f.be, tr->masks + (size_t)N * f.mask, f.y, tr->mean + f.st, tr->rstd + f.st,
                         tr->B + f.rm, tr->B + f.rv, N, f.out, eps, mom, s);
            fin = f.y;
        }
    }
    lgt_loss(tr->logits, tr->labels, N, tr->hp, tr->loss, tr->dz, s);

    // ---------------- backward: classifier
    const float* dy = tr->dz;
    for (int k = 3; k >= 0; k--) {
        TrainFc& f = tr->fc[k];
        float* dxk = tr->dfc[0];   // never the buffer dy lives in (dz or dfc[1]): the kernel reads all of dy per output
        lgt_fc_bwd(dy, k == 0 ? pooled : tr->fc[k - 1].y, W + f.w, G + f.w, G + f.b, dxk, N, f.in, f.out, s);
        if (k > 0) {
            TrainFc& p = tr->fc[k - 1];   // dxk = gradient at p.y -> through dropout / ReLU / BN1d to p.u
            float* du = tr->dfc[1];
            lgt_bn1d_bwd(dxk, p.u, tr->mean + p.st, tr->rstd + p.st, W + p.g, W + p.be, tr->masks + (size_t)N * p.mask, du,
                         G + p.g, G + p.be, N, p.out, s);
            dy = du;
        } else {
            dy = dxk;   // gradient at the pooled features [N][F]
        }
    }
    // attention + average pool
    const TrainLayer& last = tr->layers.back();
    const float* dm = nullptr;
    if (hid) {   // dy = gradient at g2 = ca * gs
        lgt_catt_gate_bwd(dy, tr->ca_ca, tr->gap, tr->ca_dgs, tr->ca_dz2, nf, s);
        lgt_fc_bwd(tr->ca_dz2, tr->ca_r, W + tr->ca_w2, G + tr->ca_w2, G + tr->ca_b2, tr->ca_dr, N, hid, F, s);
        lgt_relu_bwd(tr->ca_dr, tr->ca_z1, tr->ca_dz1, nh, s);
        lgt_fc_bwd(tr->ca_dz1, ca_in, W + tr->ca_w1, G + tr->ca_w1, G + tr->ca_b1, tr->ca_dm, N, F, hid, s);
        dy = tr->ca_dgs;
        dm = tr->ca_dm;
    }
    lgt_att_bwd(last.out, tr->att_a, dy, W + tr->att_w, spatial, N, F, P, tr->dA[0], tr->att_part, dm, G + tr->att_w, s);   // att_b = att_w + F
    // encoder.  Main chain per layer: BN backward (reduce, dx) -> backward-data convolution; the backward-weights
    // convolution of the layer (+ the ordered sum of its pixel slices) runs beside it on the second stream.  dX is double
    // buffered: layer li's dX is rewritten by layer li-2, which first waits for layer li's backward-weights.
    hipStream_t sw = tr->side_stream ? tr->stream_w : s;
    int cur = 0;
    const int nl = (int)tr->layers.size();
    for (int li = nl - 1; li >= 0; li--) {
        TrainLayer& L = tr->layers[li];
        const float* ain = li == 0 ? tr->xin : tr->layers[li - 1].out;
        float* dXl = tr->dX[li & 1];
        if (tr->side_stream && li + 2 < nl) TR_HIP(hipStreamWaitEvent(s, tr->ev_wg[li + 2], 0));
        lgt_bn2d_bwd(L.x, tr->dA[cur], tr->mean + L.st, tr->rstd + L.st, W + L.g, W + L.be,
                     L.pool ? tr->masks + (size_t)N * L.mask : nullptr, G + L.g, G + L.be, tr->bn_part, dXl, N, L.co, L.wi, s);
        if (tr->side_stream) {
            TR_HIP(hipEventRecord(tr->ev_dx[li], s));
            TR_HIP(hipStreamWaitEvent(sw, tr->ev_dx[li], 0));
        }
        lgt_wgrad(L.wi, ain, dXl, tr->partial, G + L.w, N, L.ci, L.co, sw);
        if (tr->side_stream) TR_HIP(hipEventRecord(tr->ev_wg[li], sw));
        if (li > 0) {   // backward-data: a convolution of dX with the mirrored, channel-swapped weights
            lgt_conv(tr->conv_cut, L.wi, dXl, L.wpd, nullptr, tr->dA[cur ^ 1], N, L.co, L.ci, s);
            cur ^= 1;
        }
    }
    if (tr->side_stream)
        for (int li = 0; li < std::min(2, nl); li++) TR_HIP(hipStreamWaitEvent(s, tr->ev_wg[li], 0));   // sw is in order
    // ---------------- optimizer
    lgt_clip_adam(G, tr->n_params, W, tr->M, tr->V, tr->hp, tr->state, tr->norm_part, apply_update, s);
    TR_HIP(hipGetLastError());
    return LG_OK;
}

// One optimisation step on N samples.  x [N][9][32][32], labels [N] (0/1) and masks (NULL, or [N][mask_row] keep masks
// already scaled by 1/(1-p)) are DEVICE pointers; hp is a host struct.  apply_update = 0 computes loss and gradients only.
int lg_train_step(lg_trainer* tr, const float* x, const float* labels, int N, const float* masks, uint64_t seed,
                  const lg_train_hparams* hp, int apply_update, float* loss_host, float* grad_norm_host,
                  float* logits_dev) {
    if (!tr || !x || !labels || !hp) return LG_ERR_INVALID;
    if (N < 2 || N > tr->capN) { tr->err = "lg_train_step: N must be in [2, max_batch] (BatchNorm needs a batch)"; return LG_ERR_INVALID; }
    hipSetDevice(tr->device);
    hipStream_t s = tr->stream;
    TR_HIP(hipMemcpyAsync(tr->xin, x, (size_t)N * 9 * 1024 * 4, hipMemcpyDeviceToDevice, s));
    TR_HIP(hipMemcpyAsync(tr->labels, labels, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    if (const int rc = upload_hp(tr, hp)) return rc;
    TR_HIP(hipMemcpyAsync(tr->seed_dev, &seed, sizeof(seed), hipMemcpyHostToDevice, s));
    if (masks) TR_HIP(hipMemcpyAsync(tr->masks, masks, (size_t)N * tr->mask_row * 4, hipMemcpyDeviceToDevice, s));
    if (const int rc = zero_grads(tr)) return rc;
    const uint64_t key = (uint64_t)N | ((uint64_t)(masks ? 0 : 1) << 32) | ((uint64_t)(apply_update ? 1 : 0) << 33);
    bool launched = false;
    if (tr->use_graph) {
        auto it = tr->graphs.find(key);
        if (it == tr->graphs.end()) {
            // ~75 short launches on two streams captured once per (N, mask source, update) and replayed
            hipGraph_t g = nullptr;
            hipGraphExec_t ge = nullptr;
            if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int rc = enqueue_step(tr, N, masks == nullptr, apply_update);
                const hipError_t ee = hipStreamEndCapture(s, &g);
                if (rc == LG_OK && ee == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess)
                    it = tr->graphs.emplace(key, ge).first;
                if (g) hipGraphDestroy(g);
            }
            if (it == tr->graphs.end()) {
                (void)hipGetLastError();
                tr->use_graph = false;   // capture not available: plain launches from here on
            }
        }
        if (it != tr->graphs.end()) {
            TR_HIP(hipGraphLaunch(it->second, s));
            launched = true;
        }
    }
    if (!launched) {
        const int rc = enqueue_step(tr, N, masks == nullptr, apply_update);
        if (rc != LG_OK) return rc;
    }
    if (apply_update) tr->steps++;
    if (logits_dev) TR_HIP(hipMemcpyAsync(logits_dev, tr->logits, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    if (loss_host || grad_norm_host) {
        float l = 0.f, st[4] = {0.f, 0.f, 0.f, 0.f};
        TR_HIP(hipMemcpyAsync(&l, tr->loss, 4, hipMemcpyDeviceToHost, s));
        TR_HIP(hipMemcpyAsync(st, tr->state, 16, hipMemcpyDeviceToHost, s));
        TR_HIP(hipStreamSynchronize(s));
        if (loss_host) *loss_host = l;
        if (grad_norm_host) *grad_norm_host = st[1];
    }
    return LG_OK;
}

// fit()'s batching rule (trainer.py, train_model.py:247): batches of `batch` in drawing order, a last one of fewer than 2
// samples skipped.  Host arithmetic only.
int lg_train_epoch_plan(int64_t m, int batch, int32_t* n_steps, int32_t* last_n) {
    if (m < 0 || m > INT32_MAX || batch < 2) return LG_ERR_INVALID;
    const int64_t full = m / batch, tail = m % batch;
    const int64_t steps = full + (tail >= 2 ? 1 : 0);
    if (n_steps) *n_steps = (int32_t)steps;
    if (last_n) *last_n = (int32_t)(tail >= 2 ? tail : (full > 0 ? batch : 0));
    return LG_OK;
}

// One epoch of lg_train_step calls without the host between them (see include/leafgrasp.h).  Always plain launches.
int lg_train_epoch(lg_trainer* tr, const float* x, const float* labels, int64_t n, const int32_t* idx, int64_t m, int batch,
                   uint64_t seed, const lg_train_hparams* hp, float* losses, float* grad_norms, int64_t* correct,
                   float* logits_dev, int32_t* n_steps) {
    if (!tr || !x || !labels || !hp) return LG_ERR_INVALID;
    if (n < 0 || n > INT32_MAX || m < 0 || m > INT32_MAX || (m > 0 && !idx)) { tr->err = "lg_train_epoch: n and m must be in [0, INT32_MAX], idx given"; return LG_ERR_INVALID; }
    if (batch < 2 || batch > tr->capN) { tr->err = "lg_train_epoch: batch must be in [2, max_batch] (BatchNorm needs a batch)"; return LG_ERR_INVALID; }
    if (((uintptr_t)x & 15) != 0) { tr->err = "lg_train_epoch: x must be 16-byte aligned"; return LG_ERR_INVALID; }
    for (int64_t i = 0; i < m; i++)
        if (idx[i] < 0 || (int64_t)idx[i] >= n) { tr->err = "lg_train_epoch: idx[" + std::to_string(i) + "] outside [0, n)"; return LG_ERR_INVALID; }
    int32_t steps = 0, last = 0;
    lg_train_epoch_plan(m, batch, &steps, &last);
    if (n_steps) *n_steps = steps;
    if (correct) *correct = 0;
    if (steps == 0) return LG_OK;

    hipSetDevice(tr->device);
    hipStream_t s = tr->stream;
    // device scratch: [correct u64][losses steps][grad norms steps][idx m]; the first three come back in one copy
    const size_t res_bytes = 8 + (size_t)steps * 8, need = res_bytes + (size_t)m * 4;
    if (need > tr->epoch_bytes) {
        TR_HIP(hipStreamSynchronize(s));
        if (tr->epoch_dev) TR_HIP(hipFree(tr->epoch_dev));
        tr->epoch_dev = nullptr;
        tr->epoch_bytes = 0;
        if (hipMalloc(&tr->epoch_dev, need) != hipSuccess) { tr->epoch_dev = nullptr; tr->err = "hipMalloc failed"; return LG_ERR_NOMEM; }
        tr->epoch_bytes = need;
    }
    unsigned long long* d_correct = (unsigned long long*)tr->epoch_dev;
    float* d_losses = (float*)((char*)tr->epoch_dev + 8);
    float* d_norms = d_losses + steps;
    int32_t* d_idx = (int32_t*)((char*)tr->epoch_dev + res_bytes);
    TR_HIP(hipMemcpyAsync(d_idx, idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    TR_HIP(hipMemsetAsync(d_correct, 0, 8, s));
    if (const int rc = upload_hp(tr, hp)) return rc;
    TR_HIP(hipMemcpyAsync(tr->seed_dev, &seed, sizeof(seed), hipMemcpyHostToDevice, s));
    for (int32_t k = 0; k < steps; k++) {
        const int N = k == steps - 1 ? last : batch;
        const size_t first = (size_t)k * batch;
        lgt_gather_batch(x, labels, d_idx + first, N, tr->xin, tr->labels, s);
        if (const int rc = zero_grads(tr)) return rc;   // where lg_train_step has it
        const int rc = enqueue_step(tr, N, /*draw_masks*/ true, /*apply_update*/ 1);
        if (rc != LG_OK) return rc;
        tr->steps++;
        lgt_file_step(tr->loss, tr->state, tr->logits, tr->labels, N, (int)k, d_losses, d_norms, d_correct,
                      logits_dev ? logits_dev + first : nullptr, s);
    }
    TR_HIP(hipGetLastError());
    std::vector<unsigned char> back(res_bytes);
    TR_HIP(hipMemcpyAsync(back.data(), tr->epoch_dev, res_bytes, hipMemcpyDeviceToHost, s));
    TR_HIP(hipStreamSynchronize(s));
    if (correct) { unsigned long long c = 0; memcpy(&c, back.data(), 8); *correct = (int64_t)c; }
    if (losses) memcpy(losses, back.data() + 8, (size_t)steps * 4);
    if (grad_norms) memcpy(grad_norms, back.data() + 8 + (size_t)steps * 4, (size_t)steps * 4);
    return LG_OK;
}

// Data-parallel training: lg_train_step(apply_update = 0) leaves the rank's gradients in the flat vector below; the
// caller averages it over the ranks (RCCL all-reduce on the tensor wrapping this pointer) and calls lg_train_apply.
int lg_train_grad_buffer(lg_trainer* tr, float** dev_ptr, int64_t* n) {
    if (!tr || !dev_ptr) return LG_ERR_INVALID;
    *dev_ptr = tr->G;
    if (n) *n = (int64_t)tr->n_params;
    return LG_OK;
}

// clip_grad_norm_ + Adam on the gradient vector as it stands (train_model.py:256-258)
int lg_train_apply(lg_trainer* tr, const lg_train_hparams* hp, float* grad_norm_host) {
    if (!tr || !hp) return LG_ERR_INVALID;
    hipSetDevice(tr->device);
    hipStream_t s = tr->stream;
    if (const int rc = upload_hp(tr, hp)) return rc;
    lgt_clip_adam(tr->G, tr->n_params, tr->P_, tr->M, tr->V, tr->hp, tr->state, tr->norm_part, /*apply_update*/ 1, s);
    TR_HIP(hipGetLastError());
    tr->steps++;
    if (grad_norm_host) {
        float st[4] = {0.f, 0.f, 0.f, 0.f};
        TR_HIP(hipMemcpyAsync(st, tr->state, 16, hipMemcpyDeviceToHost, s));
        TR_HIP(hipStreamSynchronize(s));
        *grad_norm_host = st[1];
    }
    return LG_OK;
}

int lg_train_sync(lg_trainer* tr) {
    if (!tr) return LG_ERR_INVALID;
    hipSetDevice(tr->device);
    TR_HIP(hipStreamSynchronize(tr->stream));
    return LG_OK;
}

}  // extern "C"

// The trainer as lg_cnn_upload_from_trainer reads it: where every tensor of lg_cnn_weights lies in the flat vectors.
bool lg_train_view(lg_trainer* tr, LgTrainView* v) {
    if (!tr || !v || !tr->P_ || !tr->B || tr->layers.size() != (size_t)2 * tr->n_blocks || tr->layers.size() > 8) return false;
    *v = LgTrainView();
    v->device = tr->device; v->n_blocks = tr->n_blocks; v->att = tr->att; v->F = tr->F; v->hid = tr->hid;
    for (int b = 0; b < 4; b++) v->filters[b] = b < tr->n_blocks ? tr->filters[b] : 0;
    v->bn_eps = 1e-5f;   // enqueue_step's eps
    v->P = tr->P_; v->B = tr->B;
    for (size_t L = 0; L < tr->layers.size(); L++) {
        const TrainLayer& l = tr->layers[L];
        v->conv_w[L] = l.w; v->conv_b[L] = l.b; v->bn_g[L] = l.g; v->bn_b[L] = l.be; v->bn_m[L] = l.rm; v->bn_v[L] = l.rv;
    }
    v->att_w = tr->att_w; v->att_b = tr->att_b;
    v->ca_w1 = tr->ca_w1; v->ca_b1 = tr->ca_b1; v->ca_w2 = tr->ca_w2; v->ca_b2 = tr->ca_b2;
    for (int k = 0; k < 4; k++) {
        v->fc_w[k] = tr->fc[k].w; v->fc_b[k] = tr->fc[k].b;
        if (k < 3) { v->fbn_g[k] = tr->fc[k].g; v->fbn_b[k] = tr->fc[k].be; v->fbn_m[k] = tr->fc[k].rm; v->fbn_v[k] = tr->fc[k].rv; }
    }
    v->stream[0] = tr->stream; v->stream[1] = tr->stream_w;
    return true;
}
