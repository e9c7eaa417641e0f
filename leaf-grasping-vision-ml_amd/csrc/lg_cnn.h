// GraspPointCNN (scripts/utils/ml_grasp_optimizer/model.py:5-128, eval mode; the four attention types and the four
// encoder_filters configurations of the reference's sweep) on gfx950: BN folded at load, 3x3 convs as implicit GEMM on
// v_mfma_f32_32x32x2_f32 (exact fp32), fused bias+ReLU(+2x2 max-pool) epilogues.
// lg_cnn.hip: the forward kernels, their launch tables and the run path.  lg_cnn_load.hip: the layer plan, the table of weight
// buffers and the one fold (three device kernels) behind both loaders -- lg_cnn_upload stages the caller's host tensors on the
// device and then runs what lg_cnn_upload_from_trainer runs on the trainer's vectors.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/leafgrasp.h"

struct RtLayer { int cin, cout, cinp, coutp, wi; bool pool; };   // real / padded channels, image width, 2x2 pool after it

// What (n_blocks, encoder_filters) make of the network: n_blocks x [conv(cin->f), conv(f->f), pool], channels padded to the
// kernels' 64-channel granule.  The defaults are the node's model, encoder [64,128,256].
struct LgCnnPlan {
    int n_layers = 6;             // 2 conv layers per encoder block
    RtLayer layers[8] = {};
    bool standard = true;         // encoder [64,128,256]: the direct kernels / A-B switches exist for this one only
    int F = 256, Fp = 256, npix = 16;   // final filters (real / padded), pixels of the last feature map
    size_t act_per_patch = 64 * 32 * 32;  // floats of the largest activation per patch
    int hid = 16;                 // channel attention's hidden width, F / 16
    int dims[5] = {256, 256, 128, 64, 1};   // classifier widths F, F, F / 2, F / 4, 1
};
// The plan of a model and whether the inference kernels take it (lg_cnn_load's codes and messages).  n_blocks == 0: three
// blocks of [64,128,256].  need_head: also refuse a classifier size lg_head_kernel has no instance for (a hand-off does, while
// the old model can still be kept; lg_cnn_load leaves that to the first forward).  Geometry is judged first (LG_ERR_UNSUPPORTED);
// an attention_type out of range comes last (LG_ERR_INVALID), with *p filled in.
int lg_cnn_plan(int n_blocks, const int32_t* filters, int attention_type, bool need_head, LgCnnPlan* p, std::string* err);
bool wino_supported(int cin, int cout, int wi, bool pool);   // the shapes lg_wino_kernel / lg_wino4_kernel are instantiated for
bool lg_head_supported(int F, int npix);                     // the instances of lg_head_kernel          (both: lg_cnn.hip)

// Weight buffers are allocated and freed through one table (weight_buffers, lg_cnn_load.hip) of the plan and att_type held
// here: a slot the table does not list for them is null.
struct LgCnn : LgCnnPlan {
    bool loaded = false;
    float* wconv[8] = {nullptr};  // packed [ky][kx][cin_pad][cout], BN folded (layer 0; all layers of the standard model)
    float* bconv[8] = {nullptr};
    float* uwino[8] = {nullptr};  // Winograd F(2x2,3x3) weights [cin][cout][16] (layers 1..)
    float* uwino4[8] = {nullptr}; // Winograd F(4x4,3x3) weights in lg_wino4_kernel's fragment order (layers 1..)
    bool use_f23 = false;         // LG_CNN_F23 at load time: F(2x2,3x3) kernels instead of F(4x4,3x3)
    float* att_w = nullptr;       // [256] spatial attention (1x1 conv 256 -> 1)
    float att_b = 0.f;
    int att_type = 0;             // LG_ATT_*
    float* ca_w1 = nullptr;       // channel attention: [16][256], [16], [256][16], [256]
    float* ca_b1 = nullptr;
    float* ca_w2 = nullptr;
    float* ca_b2 = nullptr;
    float* fcw[4] = {nullptr};    // transposed [in][out], BN folded (first three)
    float* fcb[4] = {nullptr};
    float* act[8] = {nullptr};    // output of layer L for capN patches: haloed planes [coutp][(wo+2)][(wo+4)] (lg_cnn.hip), the
    size_t act_per[8] = {0};      //   last layer dense [coutp][wo*wo] for the head; one buffer per layer: halos stay zero
    float* in_halo = nullptr;     // haloed copy [capN][12][34][36] (9 feature planes + 3 zero planes) of dense input patches (lg_cnn_forward through the C-ABI)
    float* zeros = nullptr;       // 4096 zero floats
    float* kpart = nullptr;       // lg_wino4_kernel: partial accumulators of items split along the input channels, one slot per workgroup
    unsigned* kflag = nullptr;    //   and the counters of the parts that have arrived
    unsigned* kerr_host = nullptr;   // set by a split item whose parts did not arrive (pinned host word; kerr_dev = its device address)
    unsigned* kerr_dev = nullptr;
    int wino_mask = 0x3f;         // bit L = layer L on Winograd (LG_CNN_DIRECT / LG_CNN_WINO_MASK at load time; bits 1..5: standard encoder only)
    int capN = 0;
    long long weight_allocs = 0;  // weight buffers either loader has allocated on this handle (0 more on an in-place refresh)
};

// Frees the loaded model first (a refused load leaves none, never refreshes in place), stages the host tensors of *w in one
// device vector, folds on the legacy default stream and synchronises it.
int lg_cnn_upload(LgCnn* c, const lg_cnn_weights* w, std::string* err);
void lg_cnn_free(LgCnn* c);   // weights and workspace
// patches: dense [N][9][32][32] (haloed_in = false) or haloed planes [N][12][34][36] (planes 9..11 and all halos zero) (what lg_select_grasp's
// gather writes directly; lg_cnn_halo_patch_floats() floats per patch)
// allow_split = false: no item of lg_wino4_kernel is split along the input channels, so a patch's logit does not depend on the
// number of patches of the call.  n_dev (device; needs haloed_in and lg_cnn_counts_on_device): the call runs on the first *n_dev
// of the N patch slots only -- N bounds the workspace, the grids and the slices; the logits of the other slots are not written.
// act_off: the first patch slot of the activation buffers this run takes (it uses [act_off, act_off + min(N, slice)) of every
// layer's).  Runs in flight at the same time on different streams must take ranges that do not meet, and lg_cnn_reserve must have
// made room for all of them before the first is queued: a run that had to grow the buffers would free what the others read.
int lg_cnn_run(LgCnn* c, const float* patches, bool haloed_in, int N, float* logits, hipStream_t s, std::string* err,
               bool allow_split = true, const int* n_dev = nullptr, int act_off = 0);
// Patch slots one run of N patches takes in the activation buffers (a slice's), and room for `slots` of them: grows the buffers
// behind a synchronise of s when they hold fewer, as the first run on a larger batch does by itself.
int lg_cnn_act_slots(int N);
int lg_cnn_reserve(LgCnn* c, int slots, hipStream_t s, std::string* err);
bool lg_cnn_counts_on_device(const LgCnn* c);
size_t lg_cnn_halo_patch_floats(void);
// after a synchronisation of the stream a forward ran on: true (once) if a split item of it gave up waiting for its parts
bool lg_cnn_take_error(LgCnn* c);

// ---- trainer -> inference hand-off on the device (lg_cnn_load_from_trainer)
// What the fold kernels need of an lg_trainer (lg_train.hip): the flat parameter / buffer vectors and the offsets of every tensor
// in them, in the order of lg_cnn_weights.  (lg_cnn_upload builds one of its staged copy of the host tensors.)
struct LgTrainView {
    int device = 0, n_blocks = 0, att = 0, F = 0, hid = 0;
    int filters[4] = {0, 0, 0, 0};
    float bn_eps = 1e-5f;                        // the eps of the training step's BatchNorms
    const float* P = nullptr;                    // flat parameters (DEVICE)
    const float* B = nullptr;                    // flat BatchNorm buffers (DEVICE)
    size_t conv_w[8] = {0}, conv_b[8] = {0}, bn_g[8] = {0}, bn_b[8] = {0};   // offsets into P
    size_t bn_m[8] = {0}, bn_v[8] = {0};                                       // offsets into B
    size_t att_w = 0, att_b = 0, ca_w1 = 0, ca_b1 = 0, ca_w2 = 0, ca_b2 = 0;   // P
    size_t fc_w[4] = {0}, fc_b[4] = {0}, fbn_g[3] = {0}, fbn_b[3] = {0};       // P
    size_t fbn_m[3] = {0}, fbn_v[3] = {0};                                     // B
    hipStream_t stream[2] = {nullptr, nullptr};  // the streams the trainer's steps run on
};
bool lg_train_view(lg_trainer* t, LgTrainView* v);
// The weights from the trainer's vectors, on stream s (the caller orders s after the trainer's streams); synchronises s before it
// returns (the spatial attention's bias comes back as one 4-byte copy).  The fold is lg_cnn_upload's, so every float equals what
// that writes for the same state.  Support is decided before anything is touched; same geometry as loaded (n_layers, layers[],
// att_type): the weight buffers are rewritten in place, nothing is freed or allocated.
int lg_cnn_upload_from_trainer(LgCnn* c, const LgTrainView* v, hipStream_t s, std::string* err);
// the weight buffer `which` (LG_CNNW_*) of layer `layer`: its device pointer and floats; false: no such buffer for this model
bool lg_cnn_weight_buffer(const LgCnn* c, int which, int layer, const float** p, size_t* n);
