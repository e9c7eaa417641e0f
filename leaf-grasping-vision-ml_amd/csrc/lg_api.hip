// C-ABI of liblgrasp.so (see include/leafgrasp.h).  Host orchestration only: workspaces, streams,
// the side-stream work beside the sweeps (orientation, border maxima, stem bits, bit-row export), per-kernel event timing.  No exceptions cross the boundary.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <atomic>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "lg_cnn.h"
#include "lg_dt.h"
#include "lg_eval.h"
#include "lg_leaf.h"
#include "lg_internal.h"
#include "lg_midrib.h"
#include "lg_mlsel.h"
#include "lg_options.h"
#include "lg_orient.h"
#include "lg_pool.h"

#define LG_VERSION_STR "leafgrasp-gfx950 0.4"


struct LgProfSlot {
    std::string name;
    std::vector<hipEvent_t> ev;  // pairs
    size_t used = 0;
    int launches = 0;
    double total_ms = 0.0;
};

struct lg_ctx {
    int device = 0;
    std::string err;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_prep = nullptr, ev_copy = nullptr;
    // sub-batch pipeline of lg_select_grasp: latency-bound stages run beside the bandwidth / MFMA bound ones
    hipStream_t s_dt[2] = {nullptr, nullptr}, s_main = nullptr, s_topk = nullptr;
    std::vector<hipEvent_t> ev_pool;  // untimed events, 6 per sub-batch
    hipEvent_t ev_begin = nullptr;
    // workspace, sized for (capB, capH, capW)
    int capB = 0, capH = 0, capW = 0, capK = 0;
    uint32_t* tmp = nullptr;
    unsigned long long *bits = nullptr, *stem = nullptr, *tilekeys = nullptr;
    uint8_t* tile_state = nullptr;   // [B][tiles]: which tiles' planes lg_final_kernel wrote (sparse planes, Plan::sparse)
    // near launch of lg_final_kernel (sparse planes): first list entry of every frame's near tiles, [B + 1], written by
    // lg_near_tiles_kernel on the caller's stream, and its pinned copy (read by enq_final behind ev_near)
    int32_t* near_off = nullptr;
    int32_t* near_off_host = nullptr;
    hipEvent_t ev_near = nullptr;    // behind lg_near_tiles_kernel (and the copy of its offsets, where one is made) on the caller's stream
    // device-side aliases of the small pinned results (LG_DIRECT_HOST=0 or an unmapped allocation: null, copies as before):
    // lg_near_tiles_kernel, lg_orient_kernel and lg_finish_kernel write near_off_host, fp_host (+ the status words) and
    // res_host themselves, 22 KB per 256 frames, and the host reads them behind the events it waits for anyway
    int32_t* near_off_host_dev = nullptr;
    LgFrameParams* fp_host_dev = nullptr;
    lg_grasp_result* res_host_dev = nullptr;
    int last_redo = 0;               // lg_debug_orient_redo: frames the last plane call analysed on the host after the orientation kernel handed them back
    int last_near_B = 0;             // lg_debug_near_tiles: frames of the last lg_select_grasp* call if it took the near launch, else 0
    uint32_t* maxfix = nullptr;
    uint8_t* mask_ws = nullptr;      // lg_select_grasp_labels: the 0 / 1 mask it derives from the labels (grown on demand)
    size_t mask_ws_cap = 0;
    // label-aware mode (lg_params.label_aware): bit rows of the other leaves [B][H][WW], their two dilations [2][B][H][WW] and
    // the frames' LG_ISO_MF words; allocated by the first call that sets the mode, grown on demand.  The two transforms live in
    // `tmp`, which the distance transform of the same call has finished with by then.
    unsigned long long *iso_others = nullptr, *iso_dil = nullptr;
    uint32_t* iso_mf = nullptr;
    size_t iso_words_cap = 0;
    int iso_B_cap = 0;
    int last_iso_B = 0, last_iso_H = 0, last_iso_W = 0;   // lg_debug_isolation_fields: shape of the last label-aware call (0: none since)
    int32_t* ids_dev = nullptr;      //   and the frames' leaf ids (device / pinned host staging)
    int32_t* ids_host = nullptr;
    int ids_cap = 0;
    LgWin* win = nullptr;           // [B] sweep windows (lg_window_kernel)
    LgFrameParams* fp_dev = nullptr;
    LgFrameParams* fp_host = nullptr;        // pinned
    unsigned long long* bits_host = nullptr;  // pinned
    unsigned long long* bits_host_dev = nullptr;  // device-side alias of bits_host (zero-copy export)
    LgWin* win_host = nullptr;                 // pinned copy of the sweep windows / bounding boxes
    float* ws_maps[LG_NUM_MAPS] = {nullptr};
    uint8_t* ws_valid = nullptr;
    int32_t *cand_xy = nullptr, *cand_n = nullptr;
    float *cand_info = nullptr, *patches = nullptr, *logits = nullptr;
    // CNN pruning (lg_select_grasp): the candidates that can still win (lg_cnn_cannot_win), found on the device behind top-k
    unsigned long long* surv_keep = nullptr;  // [B] bit i: candidate i goes through the CNN (lg_topk_kernel)
    int32_t* surv_list = nullptr;             // [B * K] patch slot -> frame * K + candidate, per sub-batch (lg_survivors_kernel)
    int32_t* surv_slot = nullptr;             // [B * K] candidate -> patch slot of its sub-batch, -1: pruned
    int32_t* surv_count = nullptr;            // [B] patches of sub-batch k (one sub-batch by default)
    long long last_scored = 0;                // lg_debug_cnn_scored: patches of the last call, when the host knows them;
    int last_scored_subs = 0;                 //   > 0: the sum of surv_count[0 .. last_scored_subs) instead
    // lg_debug_cnn_survivors: the shape of the last lg_select_grasp* call that ran the CNN (last_cnn_B = 0: none) -- frames,
    // top_k, frames per sub-batch, and whether the pass was pruned (the survivor buffers then hold that call's lists)
    int last_cnn_B = 0, last_cnn_K = 0, last_cnn_SB = 0;
    bool last_cnn_pruned = false;
    lg_grasp_result* res_dev = nullptr;       // [B] result rows written by lg_finish_kernel
    lg_grasp_result* res_host = nullptr;      // pinned copy
    // lg_select_grasp_candidates*: [cand_rows_cap] rows of lg_candidates_kernel and their pinned copy, allocated on the first such
    // call (handles that never ask for candidates do not grow)
    lg_grasp_candidate* cand_rows_dev = nullptr;
    lg_grasp_candidate* cand_rows_host = nullptr;
    size_t cand_rows_cap = 0;
    LgCnn cnn;
    LgLeafWs* leaf = nullptr;
    LgLeafProf* leaf_prof = nullptr;   // per-kernel times of the leaf stage (lg_profile_enable)
    LgOrientWs* orient = nullptr;   // device-side orientation scratch (lg_orient.hip)
    hipEvent_t ev_orient = nullptr, ev_side = nullptr, ev_search = nullptr;
    int last_dt_algo = 0;           // lg_debug_dt_search_form: the form the row search of the last call took (0: no search was queued)
    int prof_on = 0;  // 0 off, 1 every kernel (event pairs on the stream), 2 only launches that stamp their own events
    std::vector<LgProfSlot> prof;
    LgPool* pool = nullptr;
    LgOptions opt;               // the experiment switches, read ONCE at lg_create (never on the per-call path): lg_options.h
    long long last_patch_floats = 0;   // lg_debug_patch: floats of h->patches the last lg_select_grasp* call with the CNN could write (0: none)
    bool export_pending = false;   // this call's bit-row export has not been queued yet (enq_export)
    std::string orient_note;       // why the device-side orientation scratch could not be set up (host analysis is used then)
    std::atomic<bool> busy{false}; // one call in flight per handle (SURVEY 8b "Threading"): a concurrent second call gets LG_ERR_BUSY
    LgMidribWs* midrib = nullptr;  // lg_clahe / lg_detect_midrib scratch (lg_midrib.hip)
    void* eval_ws = nullptr;       // lg_eval_logits / lg_cnn_evaluate: result, chunk rows and (evaluate without logits_out) the logits
    size_t eval_cap = 0;
    // lg_select_grasp_ml*: the sample table and what follows it (lg_mlsel.h), grown on the first call that needs more; the
    // patches of one gather + CNN pass (haloed planes, halo zeroed at allocation); the sample rows; the chunk counts
    LgMlBuffers ml = {};
    size_t ml_cap_BM = 0, ml_cap_BH = 0;
    int ml_cap_B = 0;
    float* ml_patches = nullptr;
    int ml_patches_cap = 0;
    lg_ml_sample* ml_rows = nullptr;
    size_t ml_rows_cap = 0;
    int32_t* ml_counts_host = nullptr;    // pinned [B][2]: n, n_scored per frame
    int32_t* ml_chunk_host = nullptr;     // pinned: patches of every chunk, and their device copy
    int32_t* ml_chunk_dev = nullptr;
    size_t ml_chunk_cap = 0;
    hipEvent_t ev_ml = nullptr;           // behind the table kernels and the copy of the counts
    int ml_planes = 0;                    // lg_debug_ml_planes: 0 by rule, 1 deferred, 2 stored
    int ml_last_form = 0;
};

namespace {

int fail(lg_handle h, int code, const char* what, hipError_t e = hipSuccess) {
    if (h) {
        char buf[512];
        if (e != hipSuccess)
            snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        else
            snprintf(buf, sizeof(buf), "%s", what);
        h->err = buf;
    }
    return code;
}

#define LG_HIP(h, call)                                                    \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return fail(h, LG_ERR_HIP, #call, e_);       \
    } while (0)

// One call in flight per handle: the workspace, the profiling slots and the error string belong to the call that holds the
// flag.  rospy runs every subscriber callback on its own thread and the reference node guards itself with a plain bool
// (leaf_grasp_node_v3.py:104-107); here a concurrent second call on the SAME handle returns LG_ERR_BUSY without touching
// anything (handles are independent: different handles run side by side).
struct BusyGuard {
    lg_ctx* h;
    bool ok;
    explicit BusyGuard(lg_ctx* h_) : h(h_), ok(!h_->busy.exchange(true, std::memory_order_acquire)) {}
    ~BusyGuard() { if (ok) h->busy.store(false, std::memory_order_release); }
};
#define LG_ENTER(h)        \
    BusyGuard busy_guard_(h); \
    if (!busy_guard_.ok) return LG_ERR_BUSY

struct ProfScope {  // records an event pair around a launch when profiling is on
    lg_ctx* h;
    hipStream_t s;
    LgProfSlot* slot = nullptr;
    hipEvent_t e1 = nullptr;
    hipEvent_t e0 = nullptr;
    bool ext = false;  // true: the launch itself stamps e0/e1 (hipExtLaunchKernelGGL), nothing is recorded here
    ProfScope(lg_ctx* h_, const char* name, hipStream_t s_, bool ext_ = false) : h(h_), s(s_), ext(ext_) {
        if (!h->prof_on || (h->prof_on == 2 && !ext)) return;
        for (auto& p : h->prof)
            if (p.name == name) slot = &p;
        if (!slot) {
            h->prof.push_back(LgProfSlot());
            slot = &h->prof.back();
            slot->name = name;
        }
        if (slot->used + 2 > slot->ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { slot = nullptr; return; }
            slot->ev.push_back(a);
            slot->ev.push_back(b);
        }
        e0 = slot->ev[slot->used];
        if (!ext) hipEventRecord(e0, s);
        e1 = slot->ev[slot->used + 1];
        slot->used += 2;
    }
    ~ProfScope() {
        if (slot && e1 && !ext) hipEventRecord(e1, s);
    }
};

void prof_flush(lg_ctx* h) {  // resolve recorded pairs into totals (call after a synchronise)
    for (auto& p : h->prof) {
        for (size_t i = 0; i + 1 < p.used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) == hipSuccess) {
                p.total_ms += ms;
                p.launches++;
            }
        }
        p.used = 0;
    }
}

template <typename T>
hipError_t dev_alloc(T** p, size_t n) {
    return hipMalloc((void**)p, n * sizeof(T));
}

void free_ws(lg_ctx* h) {
    auto F = [](void* p) { if (p) hipFree(p); };
    F(h->tmp); F(h->bits); F(h->stem); F(h->tilekeys); F(h->tile_state); F(h->maxfix); F(h->win); F(h->fp_dev);
    for (int i = 0; i < LG_NUM_MAPS; i++) { F(h->ws_maps[i]); h->ws_maps[i] = nullptr; }
    F(h->ws_valid); F(h->cand_xy); F(h->cand_n); F(h->cand_info); F(h->patches); F(h->logits);
    F(h->surv_keep); F(h->surv_list); F(h->surv_slot); F(h->surv_count);
    F(h->near_off); h->near_off = nullptr; h->last_near_B = 0; h->last_iso_B = 0;
    h->surv_keep = nullptr; h->surv_list = h->surv_slot = h->surv_count = nullptr;
    h->last_scored = 0; h->last_scored_subs = 0; h->last_cnn_B = 0; h->last_patch_floats = 0;
    auto HF = [](void* p) { if (p) hipHostFree(p); };
    HF(h->fp_host); HF(h->bits_host); HF(h->win_host); HF(h->res_host); HF(h->near_off_host);
    h->near_off_host = nullptr;
    h->near_off_host_dev = nullptr; h->fp_host_dev = nullptr; h->res_host_dev = nullptr;
    F(h->res_dev);
    h->tmp = nullptr; h->bits = h->stem = h->tilekeys = nullptr; h->tile_state = nullptr; h->maxfix = nullptr; h->win = nullptr; h->fp_dev = nullptr;
    h->ws_valid = nullptr; h->cand_xy = h->cand_n = nullptr; h->cand_info = h->patches = h->logits = nullptr;
    h->fp_host = nullptr; h->bits_host = nullptr; h->win_host = nullptr; h->bits_host_dev = nullptr; h->res_dev = h->res_host = nullptr;
    h->capB = h->capH = h->capW = h->capK = 0;
}

int ensure_ws(lg_ctx* h, int B, int H, int W, int K) {
    if (B <= h->capB && H == h->capH && W == h->capW && K <= h->capK) return LG_OK;
    int nB = std::max(B, h->capB), nK = std::max(K, std::max(h->capK, 20));
    hipDeviceSynchronize();
    free_ws(h);
    const size_t px = (size_t)nB * H * W;
    const int WW = (W + 63) / 64;
    const size_t words = (size_t)nB * H * WW;
    const int tiles = ((W + LG_TW - 1) / LG_TW) * ((H + LG_TH - 1) / LG_TH);
    LG_HIP(h, dev_alloc(&h->tmp, px * 2));
    LG_HIP(h, dev_alloc(&h->bits, words));
    LG_HIP(h, dev_alloc(&h->stem, words));
    LG_HIP(h, dev_alloc(&h->tilekeys, (size_t)nB * tiles));
    LG_HIP(h, dev_alloc(&h->tile_state, (size_t)nB * tiles));
    LG_HIP(h, dev_alloc(&h->near_off, (size_t)nB + 1));
    LG_HIP(h, hipHostMalloc((void**)&h->near_off_host, sizeof(int32_t) * ((size_t)nB + 1)));
    LG_HIP(h, dev_alloc(&h->maxfix, (size_t)nB * LG_MF));
    LG_HIP(h, dev_alloc(&h->win, (size_t)nB));
    LG_HIP(h, dev_alloc(&h->fp_dev, (size_t)nB));
    LG_HIP(h, hipHostMalloc((void**)&h->fp_host, sizeof(LgFrameParams) * nB));
    LG_HIP(h, hipHostMalloc((void**)&h->win_host, sizeof(LgWin) * nB));
    LG_HIP(h, hipHostMalloc((void**)&h->bits_host, sizeof(unsigned long long) * words));
    // device-side alias of the pinned image: lg_export_rows_kernel posts only the bounding-box bits into it.
    // An unmapped allocation: whole-batch hipMemcpyAsync instead.
    if (hipHostGetDevicePointer((void**)&h->bits_host_dev, h->bits_host, 0) != hipSuccess)
        h->bits_host_dev = nullptr;   // fall back to a full-batch hipMemcpyAsync
    LG_HIP(h, dev_alloc(&h->ws_valid, px));   // validity plane for callers that do not want it back
    LG_HIP(h, dev_alloc(&h->cand_xy, (size_t)nB * nK * 2));
    LG_HIP(h, dev_alloc(&h->cand_n, (size_t)nB));
    LG_HIP(h, dev_alloc(&h->cand_info, (size_t)nB * nK * 2));
    // candidate patches as haloed planes (the CNN's staging layout); the halo is zeroed here, once
    LG_HIP(h, dev_alloc(&h->patches, (size_t)nB * nK * lg_cnn_halo_patch_floats()));
    LG_HIP(h, hipMemset(h->patches, 0, (size_t)nB * nK * lg_cnn_halo_patch_floats() * sizeof(float)));
    LG_HIP(h, dev_alloc(&h->logits, (size_t)nB * nK));
    LG_HIP(h, dev_alloc(&h->surv_keep, (size_t)nB));
    LG_HIP(h, dev_alloc(&h->surv_list, (size_t)nB * nK));
    LG_HIP(h, dev_alloc(&h->surv_slot, (size_t)nB * nK));
    LG_HIP(h, dev_alloc(&h->surv_count, (size_t)nB));
    LG_HIP(h, dev_alloc(&h->res_dev, (size_t)nB));
    LG_HIP(h, hipHostMalloc((void**)&h->res_host, sizeof(lg_grasp_result) * nB));
    if (h->opt.direct_host) {
        if (hipHostGetDevicePointer((void**)&h->near_off_host_dev, h->near_off_host, 0) != hipSuccess) h->near_off_host_dev = nullptr;
        if (hipHostGetDevicePointer((void**)&h->fp_host_dev, h->fp_host, 0) != hipSuccess) h->fp_host_dev = nullptr;
        if (hipHostGetDevicePointer((void**)&h->res_host_dev, h->res_host, 0) != hipSuccess) h->res_host_dev = nullptr;
        (void)hipGetLastError();   // (a refused alias only means the copy is made)
    }
    if (!h->opt.host_orient && H <= 16384 && W <= 8192) {
        // no device-side scratch (allocation, or the LDS request on a part with less of it): the host contour analysis of
        // every frame is a complete path of its own -- scoring goes on, the reason stays readable in orient_note
        std::string err;
        // (LG_ORIENT_FAIL makes the set-up fail -- the test of this hand-over)
        if (h->opt.orient_fail || lg_orient_ensure(h->orient, nB, H, h->opt.orient_cap, &err)) {
            h->orient_note = err.empty() ? "orientation scratch: LG_ORIENT_FAIL is set" : err;
            lg_orient_free(h->orient);
            (void)hipGetLastError();   // the failed allocation's error is sticky until read: it must not fail the call that goes on without it
        }
    } else {
        lg_orient_free(h->orient);   // (a scratch sized for another image height must not outlive it: host analysis from here on)
    }
    h->capB = nB; h->capH = H; h->capW = W; h->capK = nK;
    return LG_OK;
}

int ensure_ws_map(lg_ctx* h, int i) {  // internal plane when the caller does not want map i
    if (h->ws_maps[i]) return LG_OK;
    LG_HIP(h, dev_alloc(&h->ws_maps[i], (size_t)h->capB * h->capH * h->capW));
    return LG_OK;
}

// ImageProcessor._create_gaussian_kernel (image_processor.py:25-32): the 2-D kernel exp(-(dx^2 + dy^2) / 2 sigma^2) / sum with
// sigma = size / 6 is the outer product of this 1-D factor with itself
void gaussian1d(int size, float* k1) {
    const double sigma = size / 6.0;
    const int c = size / 2;
    double e[LG_MAX_GAUSS], s = 0;
    for (int i = 0; i < size; i++) { e[i] = exp(-((i - c) * (i - c)) / (2 * sigma * sigma)); s += e[i]; }
    for (int i = 0; i < size; i++) k1[i] = (float)(e[i] / s);
}

void ml_free(lg_ctx* h) {
    auto F = [](void* p) { if (p) hipFree(p); };
    LgMlBuffers& m = h->ml;
    F(m.frames); F(m.row_pre); F(m.xy); F(m.scored); F(m.slot_local); F(m.list); F(m.slot); F(m.counts); F(m.n_frame); F(m.logits);
    F(m.pick_n); F(m.pick_xy); F(m.pick_info); F(m.pick_meta);
    m = LgMlBuffers{};
    h->ml_cap_BM = h->ml_cap_BH = 0; h->ml_cap_B = 0;
    F(h->ml_patches); h->ml_patches = nullptr; h->ml_patches_cap = 0;
    F(h->ml_rows); h->ml_rows = nullptr; h->ml_rows_cap = 0;
    F(h->ml_chunk_dev); h->ml_chunk_dev = nullptr;
    if (h->ml_counts_host) hipHostFree(h->ml_counts_host);
    if (h->ml_chunk_host) hipHostFree(h->ml_chunk_host);
    h->ml_counts_host = h->ml_chunk_host = nullptr; h->ml_chunk_cap = 0;
}

void parallel_for(lg_ctx* h, int n, const std::function<void(int)>& fn) {
    if (h->pool && n > 1) h->pool->run(n, fn);
    else
        for (int i = 0; i < n; i++) fn(i);
}

}  // namespace

extern "C" {

const char* lg_version(void) { return LG_VERSION_STR; }

void lg_default_params(lg_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->cx = 707.0; p->cy = 494.0; p->f = 0.0;  // grasp_point_selector.py:29-31 (f_norm unset)
    p->w_approach = 0.4f; p->w_sdf = 0.3f; p->w_flat = 0.2f; p->w_access = 0.1f;
    p->sdf_w_interior = 0.4f; p->sdf_w_align = 0.4f; p->sdf_w_sdf = 0.2f;
    p->optimal_distance = 20.f;
    p->access_w_dist = 0.7f; p->access_w_dir = 0.3f;
    p->flat_scale = 5.f;
    p->iso_w_close = 0.7f; p->iso_w_wide = 0.3f;
    p->iso_ramp_top = 1.0f; p->iso_ramp_bottom = 0.2f;
    p->min_edge_distance = 20.f; p->stem_valid_thresh = 0.8f;
    p->stem_se = 30; p->stem_bottom_div = 3;
    p->top_k = 20; p->nms_min_distance = 10;
    p->pregrasp_clearance = 15;
    p->mask_is_bool = 1;
    p->gaussian_size = 5;   // the node's ImageProcessor(..., gaussian_kernel_size=5) (leaf_grasp_node_v3.py:37,66-67)
    p->chamfer_init_dist0 = (int32_t)LG_INIT0;   // INT_MAX >> 2
}

static thread_local std::string g_create_err = "null handle";

int lg_create(int device, lg_handle* out) {
    if (!out) return LG_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    {
        const hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || device < 0 || device >= n) {
            g_create_err = std::string("lg_create: hipGetDeviceCount -> ") + hipGetErrorString(e) + ", " + std::to_string(n) +
                           " device(s), asked for " + std::to_string(device);
            return LG_ERR_HIP;
        }
    }
    lg_ctx* h = new (std::nothrow) lg_ctx();
    if (!h) return LG_ERR_NOMEM;
    h->device = device;
    // The side stream is created with the highest priority: ROCm multiplexes normal-priority streams onto a few
    // in-order hardware queues, and when the side stream lands on the caller's queue the 0.65 ms bit-row export
    // sits between pack_bits and the sweeps (measured: sweeps finish at 2.4 ms instead of 1.8 ms at B=128).
    // Priority streams get hardware queues of their own.
    int prio_least = 0, prio_greatest = 0;
    if (hipSetDevice(device) == hipSuccess) hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithPriority(&h->copy_stream, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_prep, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_copy, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_orient, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_side, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_search, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_near, hipEventDisableTiming) != hipSuccess) {
        g_create_err = std::string("lg_create: stream / event creation -> ") + hipGetErrorString(hipGetLastError());
        delete h;
        return LG_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&h->s_dt[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->s_dt[1], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->s_main, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->s_topk, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_begin, hipEventDisableTiming) != hipSuccess) {
        g_create_err = std::string("lg_create: stream / event creation -> ") + hipGetErrorString(hipGetLastError());
        delete h;
        return LG_ERR_HIP;
    }
    h->opt = lg_options_from_env();
    h->pool = new (std::nothrow) LgPool(h->opt.host_threads - 1);  // the calling thread is the last worker
    h->leaf_prof = lg_leaf_prof_new();
    *out = h;
    return LG_OK;
}

int lg_destroy(lg_handle h) {
    if (!h) return LG_ERR_INVALID;
    if (h->busy.exchange(true, std::memory_order_acquire)) return LG_ERR_BUSY;   // a call is running on another thread
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    delete h->pool;
    h->pool = nullptr;
    free_ws(h);
    if (h->mask_ws) hipFree(h->mask_ws);
    if (h->ids_dev) hipFree(h->ids_dev);
    if (h->ids_host) hipHostFree(h->ids_host);
    if (h->iso_others) hipFree(h->iso_others);
    if (h->iso_dil) hipFree(h->iso_dil);
    if (h->iso_mf) hipFree(h->iso_mf);
    if (h->cand_rows_dev) hipFree(h->cand_rows_dev);
    if (h->cand_rows_host) hipHostFree(h->cand_rows_host);
    lg_cnn_free(&h->cnn);
    if (h->eval_ws) hipFree(h->eval_ws);
    ml_free(h);
    if (h->ev_ml) hipEventDestroy(h->ev_ml);
    lg_leaf_free(h->leaf);
    lg_leaf_prof_free(h->leaf_prof);
    lg_orient_free(h->orient);
    lg_midrib_free(h->midrib);
    if (h->ev_orient) hipEventDestroy(h->ev_orient);
    if (h->ev_side) hipEventDestroy(h->ev_side);
    if (h->ev_search) hipEventDestroy(h->ev_search);
    if (h->ev_near) hipEventDestroy(h->ev_near);
    for (auto& p : h->prof)
        for (auto e : p.ev) hipEventDestroy(e);
    for (auto e : h->ev_pool) hipEventDestroy(e);
    if (h->ev_begin) hipEventDestroy(h->ev_begin);
    for (hipStream_t q : {h->s_dt[0], h->s_dt[1], h->s_main, h->s_topk})
        if (q) hipStreamDestroy(q);
    if (h->ev_prep) hipEventDestroy(h->ev_prep);
    if (h->ev_copy) hipEventDestroy(h->ev_copy);
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    delete h;
    return LG_OK;
}

const char* lg_last_error(lg_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }   // NULL: why lg_create failed

const char* lg_orientation_note(lg_handle h) { return h ? h->orient_note.c_str() : ""; }

int lg_profile_enable(lg_handle h, int on) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    for (auto& p : h->prof) { p.used = 0; p.launches = 0; p.total_ms = 0.0; }
    h->prof_on = on < 0 ? 0 : on;
    lg_leaf_prof_enable(h->leaf_prof, on == 1);
    return LG_OK;
}

int lg_profile_read(lg_handle h, const char* name, int* launches, double* total_ms) {
    if (!h || !name) return LG_ERR_INVALID;
    LG_ENTER(h);
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    prof_flush(h);
    if (launches) *launches = 0;
    if (total_ms) *total_ms = 0.0;
    if (lg_leaf_prof_read(h->leaf_prof, name, launches, total_ms)) return LG_OK;
    for (auto& p : h->prof)
        if (p.name == name) {
            if (launches) *launches = p.launches;
            if (total_ms) *total_ms = p.total_ms;
            return LG_OK;
        }
    return LG_OK;
}

int lg_debug_dt_max(lg_handle h, int frame, uint32_t out[2], int32_t win[4]) {
    if (!h || !out || frame < 0 || frame >= h->capB || !h->maxfix) return LG_ERR_INVALID;
    LG_ENTER(h);
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (hipMemcpy(out, h->maxfix + LG_MF * (size_t)frame, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_dt_max: copy failed");
    if (win) {
        LgWin w;
        if (hipMemcpy(&w, h->win + frame, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(h, LG_ERR_HIP, "lg_debug_dt_max: copy failed");
        win[0] = w.wx0; win[1] = w.wx0 + w.nw * lg_dt_geometry(h->capW, nullptr); win[2] = w.wy0; win[3] = w.wy1;
        if (win[1] > h->capW) win[1] = h->capW;
    }
    return LG_OK;
}

int lg_debug_cnn_scored(lg_handle h, int64_t* patches) {
    if (!h || !patches) return LG_ERR_INVALID;
    LG_ENTER(h);
    long long n = h->last_scored;
    if (h->last_scored_subs > 0) {
        if (!h->surv_count || h->last_scored_subs > h->capB) return LG_ERR_INVALID;
        hipSetDevice(h->device);
        hipDeviceSynchronize();
        std::vector<int32_t> c((size_t)h->last_scored_subs);
        if (hipMemcpy(c.data(), h->surv_count, sizeof(int32_t) * c.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(h, LG_ERR_HIP, "lg_debug_cnn_scored: copy failed");
        n = 0;
        for (int32_t v : c) n += v;
    }
    *patches = n;
    return LG_OK;
}

int lg_debug_leaf_fallback(lg_handle h, int32_t* flags, int cap, int32_t* n_frames, int32_t* n_flagged) {
    if (!h || !n_frames || !n_flagged || cap < 0 || (cap > 0 && !flags)) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (lg_leaf_last_fallback(h->leaf, flags, cap, n_frames, n_flagged))
        return fail(h, LG_ERR_INVALID, "lg_debug_leaf_fallback: cap is smaller than the last call's batch");
    return LG_OK;
}

int lg_debug_cnn_survivors(lg_handle h, int32_t* sub_frames, int32_t* n_sub, int32_t* counts, int32_t counts_cap,
                           int32_t* list, int32_t* slot, float* logits, int64_t cap, int64_t* n_slots) {
    if (!h || !sub_frames || !n_sub || !n_slots) return LG_ERR_INVALID;
    const bool query = !counts && !list && !slot && !logits && counts_cap == 0 && cap == 0;   // sizes only
    if (!query && (!counts || !list || !slot || !logits)) return LG_ERR_INVALID;
    LG_ENTER(h);
    const int B = h->last_cnn_B, K = h->last_cnn_K, SB = h->last_cnn_SB;
    if (B <= 0 || K <= 0 || SB <= 0 || B > h->capB || K > h->capK || !h->logits || !h->surv_count)
        return fail(h, LG_ERR_INVALID, "lg_debug_cnn_survivors: no lg_select_grasp call with the CNN on this workspace");
    const int nsub = (B + SB - 1) / SB;
    const size_t total = (size_t)B * K;
    *sub_frames = SB; *n_sub = nsub; *n_slots = (int64_t)total;
    if (query) return LG_OK;
    if (counts_cap < nsub || cap < 0 || (size_t)cap < total)
        return fail(h, LG_ERR_INVALID, "lg_debug_cnn_survivors: output arrays too small");
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (hipMemcpy(logits, h->logits, sizeof(float) * total, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_cnn_survivors: copy failed");
    if (h->last_cnn_pruned) {
        if (hipMemcpy(counts, h->surv_count, sizeof(int32_t) * nsub, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(list, h->surv_list, sizeof(int32_t) * total, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(slot, h->surv_slot, sizeof(int32_t) * total, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(h, LG_ERR_HIP, "lg_debug_cnn_survivors: copy failed");
    }
    for (int k = 0; k < nsub; k++) {
        const int off = k * SB, n = std::min(SB, B - off);
        int32_t* const l = list + (size_t)off * K;
        const int32_t slots = n * K;
        if (!h->last_cnn_pruned) {   // every candidate has a patch, in its own place
            counts[k] = slots;
            for (int32_t j = 0; j < slots; j++) l[j] = slot[(size_t)off * K + j] = j;
        } else {                     // (the device wrote the first counts[k] entries of the list only)
            const int32_t c = std::max(0, std::min(counts[k], slots));
            for (int32_t j = c; j < slots; j++) l[j] = -1;
        }
    }
    return LG_OK;
}

int lg_debug_patch(lg_handle h, int64_t slot, float* out) {
    if (!h || !out || slot < 0) return LG_ERR_INVALID;
    LG_ENTER(h);
    const long long pf = lg_cnn_halo_patch_floats();   // [12][34][36], pixel (y, x) at [y + 1][x + 1]
    if (!h->patches || (slot + 1) * pf > h->last_patch_floats)
        return fail(h, LG_ERR_INVALID, "lg_debug_patch: no such patch slot in the last lg_select_grasp call with the CNN on this workspace");
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    std::vector<float> buf((size_t)pf);
    if (hipMemcpy(buf.data(), h->patches + (size_t)slot * pf, sizeof(float) * pf, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_patch: copy failed");
    for (int c = 0; c < 9; c++)
        for (int y = 0; y < 32; y++)
            memcpy(out + ((size_t)c * 32 + y) * 32, buf.data() + ((size_t)c * 34 + y + 1) * 36 + 1, sizeof(float) * 32);
    return LG_OK;
}

int lg_debug_ws_plane_bytes(lg_handle h, int64_t bytes[LG_NUM_MAPS]) {
    if (!h || !bytes) return LG_ERR_INVALID;
    LG_ENTER(h);
    for (int i = 0; i < LG_NUM_MAPS; i++)
        bytes[i] = h->ws_maps[i] ? (int64_t)sizeof(float) * h->capB * h->capH * h->capW : 0;
    return LG_OK;
}

int lg_wave_rows_on_mask(const uint64_t* bits, int H, int WW, int y, int w) {
    if (!bits || H < 1 || WW < 1 || y < 0 || y >= H || w < 0 || w >= WW) return LG_ERR_INVALID;
    return lg_wave_on_mask((const unsigned long long*)bits, H, WW, y, w) ? 1 : 0;
}

int lg_near_tile_rect(int bx0, int bx1, int by0, int by1, int H, int W, int halo, int32_t rect[4]) {
    if (!rect || H < 1 || W < 1 || halo < 0) return LG_ERR_INVALID;
    int r[4];
    const int n = lg_near_tiles(bx0, bx1, by0, by1, H, W, halo, &r[0], &r[1], &r[2], &r[3]);
    for (int i = 0; i < 4; i++) rect[i] = r[i];
    return n;
}

int lg_stem_plan(int k, int n, int anchor, const int8_t* lo, const int8_t* hi, int32_t* i0, int8_t span_lo[64], int8_t span_hi[64],
                 int8_t dlo[64], int8_t dhi[64]) {
    LgSeSpans se;
    if (k >= 1 && k <= 64) {
        lg_make_se_spans(k, &se);
    } else {
        if (k != 0 || !lo || !hi || n < 1 || n > 64 || anchor < 0 || anchor >= n) return LG_ERR_INVALID;
        memset(&se, 0, sizeof(se));
        se.n = n; se.anchor = anchor;
        for (int i = 0; i < n; i++) {
            if (lo[i] < -32 || lo[i] > 32 || hi[i] < -32 || hi[i] > 32 || hi[i] - lo[i] > 62) return LG_ERR_INVALID;
            se.lo[i] = lo[i]; se.hi[i] = hi[i];
        }
    }
    LgStemPlan sp;
    lg_make_stem_plan(se, &sp);
    if (i0) *i0 = sp.i0;
    for (int i = 0; i < 64; i++) {
        if (span_lo) span_lo[i] = i < se.n ? se.lo[i] : 0;
        if (span_hi) span_hi[i] = i < se.n ? se.hi[i] : 0;
        if (dlo) dlo[i] = sp.dlo[i];
        if (dhi) dhi[i] = sp.dhi[i];
    }
    return sp.nested;
}

namespace {
// a frame's stem words on the host, laid out as the kernels lay them out: the nested-span form on the words of the bounding box
// (zeros elsewhere), or the per-row form on every word.  Returns 1 when the chains ran, 0 for the per-row loop.
int stem_words_host(const unsigned long long* bits, int H, int W, int WW, int bottom_start, const LgSeSpans& se, int algo,
                    unsigned long long* out) {
    LgStemPlan sp;
    lg_make_stem_plan(se, &sp);
    if (!algo || !sp.nested) {
        for (int y = 0; y < H; y++)
            for (int w = 0; w < WW; w++) {
                const unsigned long long self = bits[(size_t)y * WW + w];
                unsigned long long acc = 0;
                if (self != 0 && y + (se.n - 1 - se.anchor) >= bottom_start) acc = lg_stem_word_rows(bits, H, WW, bottom_start, y, w, se);
                out[(size_t)y * WW + w] = acc & self;
            }
        return 0;
    }
    LgWin wn;
    memset(&wn, 0, sizeof(wn));
    wn.bx0 = W; wn.bx1 = -1; wn.by0 = H; wn.by1 = -1;
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) {
            const unsigned long long v = bits[(size_t)y * WW + w];
            if (!v) continue;
            wn.bx0 = std::min(wn.bx0, 64 * w + __builtin_ctzll(v));
            wn.bx1 = std::max(wn.bx1, 64 * w + 63 - __builtin_clzll(v));
            wn.by0 = std::min(wn.by0, y);
            wn.by1 = y;
        }
    const LgStemRect rc = lg_stem_active(wn, H, WW, bottom_start, se.n, se.anchor);
    const int ya = rc.ya, yb = rc.yb, w0 = rc.w0, w1 = rc.w1;
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) {
            const size_t o = (size_t)y * WW + w;
            if (!(y >= ya && y <= yb && w >= w0 && w <= w1)) { out[o] = 0ull; continue; }
            const unsigned long long self = bits[o];
            out[o] = self ? (lg_stem_word_chain(bits, H, WW, bottom_start, y, w, se, sp) & self) : 0ull;
        }
    return 1;
}
}  // namespace

int lg_stem_words_host(const uint64_t* bits, int H, int W, int WW, int bottom_start, int k, uint64_t* out) {
    if (!bits || !out || H < 1 || W < 1 || WW != (W + 63) / 64 || bottom_start < 0 || bottom_start > H || k < 1 || k > 64)
        return LG_ERR_INVALID;
    LgSeSpans se;
    lg_make_se_spans(k, &se);
    return stem_words_host((const unsigned long long*)bits, H, W, WW, bottom_start, se, 1, (unsigned long long*)out);
}

int lg_stem_words_host_spans(const uint64_t* bits, int H, int W, int WW, int bottom_start, int n, int anchor, const int8_t* lo,
                             const int8_t* hi, int algo, uint64_t* out) {
    if (!bits || !out || !lo || !hi || H < 1 || W < 1 || WW != (W + 63) / 64 || bottom_start < 0 || bottom_start > H || n < 1 ||
        n > 64 || anchor < 0 || anchor >= n)
        return LG_ERR_INVALID;
    LgSeSpans se;
    memset(&se, 0, sizeof(se));
    se.n = n; se.anchor = anchor;
    for (int i = 0; i < n; i++) {
        if (lo[i] < -32 || lo[i] > 32 || hi[i] < -32 || hi[i] > 32 || hi[i] - lo[i] > 62) return LG_ERR_INVALID;
        se.lo[i] = lo[i]; se.hi[i] = hi[i];
    }
    return stem_words_host((const unsigned long long*)bits, H, W, WW, bottom_start, se, algo, (unsigned long long*)out);
}

int lg_window_from_box(const uint32_t box[5], int H, int W, int search_mode, int32_t out[12]) {
    int nw = 0;
    const int wc = (H >= 1 && W >= 1) ? lg_dt_geometry(W, &nw) : 0;
    if (!box || !out || wc == 0 || search_mode < 0 || search_mode > 2) return LG_ERR_INVALID;
    if (box[4] != 0 && (box[0] >= (uint32_t)W || box[1] >= (uint32_t)W || box[2] >= (uint32_t)H || box[3] >= (uint32_t)H)) return LG_ERR_INVALID;
    const LgWin w = lg_win_from_box(box, H, W, wc, nw, search_mode);
    out[0] = w.wx0; out[1] = std::min(W, w.wx0 + w.nw * wc); out[2] = w.wy0; out[3] = w.wy1;
    out[4] = w.bx0; out[5] = w.bx1; out[6] = w.by0; out[7] = w.by1;
    out[8] = w.skip_out; out[9] = w.search_in; out[10] = w.area; out[11] = wc;
    return LG_OK;
}

int lg_border_line_max(const int32_t* prof, int n, int lo, int len, uint32_t* out) {
    if (!prof || !out || n < 1 || lo < 0 || len > 16384 || lo > len - n) return LG_ERR_INVALID;
    for (int i = 0; i < n; i++)
        if (prof[i] < -1 || prof[i] > 16384) return LG_ERR_INVALID;   // (the norm of two such lengths stays below 2^32)
    lg_border_search(prof, n, lo, len, out);
    return LG_OK;
}

int lg_debug_near_tiles(lg_handle h, int32_t* off, int cap) {
    if (!h || !off) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (h->last_near_B <= 0 || !h->near_off_host) return fail(h, LG_ERR_INVALID, "lg_debug_near_tiles: the last call did not take the near launch");
    if (cap < h->last_near_B + 1) return fail(h, LG_ERR_INVALID, "lg_debug_near_tiles: cap must hold B + 1 entries");
    memcpy(off, h->near_off_host, sizeof(int32_t) * (h->last_near_B + 1));   // (the call that wrote it has been synchronised)
    return LG_OK;
}

int lg_debug_orient_redo(lg_handle h, int32_t* n) {
    if (!h || !n) return LG_ERR_INVALID;
    LG_ENTER(h);
    *n = h->last_redo;
    return LG_OK;
}

int lg_debug_options(lg_handle h, char* buf, int cap) {
    if (!h) return LG_ERR_INVALID;
    return lg_options_print(h->opt, buf, cap);   // (written once, by lg_create: no call in flight changes it)
}

int lg_debug_dt_form(lg_handle h, int frame, int32_t form[2]) {
    if (!h || !form || frame < 0 || frame >= h->capB || !h->win) return LG_ERR_INVALID;
    LG_ENTER(h);
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    LgWin w;
    if (hipMemcpy(&w, h->win + frame, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_dt_form: copy failed");
    form[0] = w.search_in ? 1 : 0;
    form[1] = w.skip_out ? 1 : 0;
    return LG_OK;
}

int lg_debug_dt_search_form(lg_handle h, int32_t* algo) {
    if (!h || !algo) return LG_ERR_INVALID;
    LG_ENTER(h);
    *algo = h->last_dt_algo;
    return LG_OK;
}

int lg_dt_form_host(int forced, int n, int H, int W) { return lg_dt_form(forced, n, H, W); }

int lg_debug_isolation_fields(lg_handle h, int frame, uint32_t* dc_fix, uint32_t* dw_fix, uint32_t max_fix[2]) {
    if (!h || !max_fix || frame < 0) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (frame >= h->last_iso_B || !h->tmp || !h->iso_mf)
        return fail(h, LG_ERR_INVALID, "lg_debug_isolation_fields: the last call on this workspace was not label-aware, or has no such frame");
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    uint32_t mf[LG_ISO_MF];
    if (hipMemcpy(mf, h->iso_mf + LG_ISO_MF * (size_t)frame, sizeof(mf), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_isolation_fields: copy failed");
    if (mf[2] == 0u) return 0;   // no other leaf: the closed form, no fields
    max_fix[0] = mf[0]; max_fix[1] = mf[1];
    const size_t px = (size_t)h->last_iso_H * h->last_iso_W;
    uint32_t* dst[2] = {dc_fix, dw_fix};
    for (int f = 0; f < 2; f++)
        if (dst[f] && hipMemcpy(dst[f], h->tmp + ((size_t)frame * 2 + f) * px, sizeof(uint32_t) * px, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(h, LG_ERR_HIP, "lg_debug_isolation_fields: copy failed");
    return 1;
}

int lg_label_aware_check(const lg_params* p, int has_labels) {
    if (!p || (p->label_aware != 0 && p->label_aware != 1)) return LG_ERR_INVALID;
    return (p->label_aware && !has_labels) ? LG_ERR_INVALID : LG_OK;
}

int lg_norm3_host(const int32_t* dx, const int32_t* dy, int n, uint32_t* out) {
    if (n < 0 || (n > 0 && (!dx || !dy || !out))) return LG_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        const int ax = dx[i] < 0 ? -dx[i] : dx[i], ay = dy[i] < 0 ? -dy[i] : dy[i];
        if (ax > 16384 || ay > 16384) return LG_ERR_INVALID;   // (the norm of two such lengths stays below 2^32)
        out[i] = lg_norm3(ax, ay);
    }
    return LG_OK;
}

int lg_dilate_words_host(const uint64_t* bits, int H, int W, int WW, int k, uint64_t* out) {
    if (!bits || !out || H < 1 || W < 1 || WW != (W + 63) / 64 || k < 1 || k > 64) return LG_ERR_INVALID;
    LgSeSpans se;
    lg_make_se_spans(k, &se);
    LgStemPlan sp;
    lg_make_stem_plan(se, &sp);
    // (bits past W are ignored: the source rows are taken with their last word masked)
    std::vector<unsigned long long> src((size_t)H * WW);
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) {
            unsigned long long v = (unsigned long long)bits[(size_t)y * WW + w];
            if (w == WW - 1 && (W & 63)) v &= ~0ull >> (64 - (W & 63));
            src[(size_t)y * WW + w] = v;
        }
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) out[(size_t)y * WW + w] = lg_frame_dilate_word(src.data(), H, W, WW, y, w, se, sp);
    return LG_OK;
}

}  // extern "C"

namespace {

struct Plan {  // one call's geometry, parameters and plane pointers (absolute, frame 0)
    int B, H, W, WW, tiles_x, tiles_y;
    lg_params P;
    const float* depth;
    const uint8_t* mask;
    const int16_t* labels = nullptr;   // lg_select_grasp_labels: mask (the handle's workspace) is written from these by the bit-row pass
    float* maps[LG_NUM_MAPS];
    uint8_t* valid;
    // sparse planes: the caller takes no plane and no validity back (lg_select_grasp*): constant tiles of the workspace planes
    // stay unwritten, lg_final_kernel records per tile which were written (tile_state), top-k and the gather read that
    bool sparse = false;
    // near launch: lg_final_kernel takes only the tiles around the leaves (lg_near_tiles), the others get their constant key and
    // state byte from lg_near_tiles_kernel beside the distance transform.  Sparse mode, one sub-batch, constant-tile path on.
    bool near = false;
    // deferred planes (sparse mode, unless LG_DEFER_PLANES=0): lg_final_kernel stores what top-k reads and flatness (score-only);
    // sdf, approach, isolation, accessibility and stem are neither allocated nor written: the gather computes them at the
    // pixels of its windows
    bool defer = false;
    // label-aware mode (lg_params.label_aware, labels given): the bit-row pass also writes the other leaves' rows (iso_others)
    bool label_aware = false;
};


// frame-border maxima of d_out + stem bits: both read only the bit rows, neither is needed before the plane kernel
int enq_tail(lg_ctx* h, const Plan& pl, int off, int n, hipStream_t s) {
    const size_t words = (size_t)pl.H * pl.WW;
    {
        ProfScope ps(h, "dt_border", s);
        lg_launch_dout_border(h->bits + off * words, h->win + off, h->maxfix + LG_MF * (size_t)off, n, pl.H, pl.W, pl.WW, s);
    }
    // (on the side stream both run before the bit-row export, which slows every concurrent memory-bound kernel 4x)
    {
        LgSeSpans se;
        lg_make_se_spans(pl.P.stem_se, &se);
        // bottom[-third:, :] = 1 (:693-694): a frame shorter than the divisor has third == 0, and numpy's [-0:] is every row
        const int third = pl.H / pl.P.stem_bottom_div;
        // two chains of nested spans on the words of the bounding boxes; spans that are not nested (no ellipse gives any), or
        // LG_STEM_ALGO=0: the per-row kernel
        LgStemPlan sp;
        lg_make_stem_plan(se, &sp);
        ProfScope ps(h, "stem", s);
        lg_launch_stem_bits(h->bits + off * words, h->stem + off * words, h->win + off, n, pl.H, pl.W, pl.WW,
                            third ? pl.H - third : 0, se, h->opt.stem_algo ? &sp : nullptr, s);
    }
    return LG_OK;
}

// pack bits + D2H of the bit rows on the copy stream
int enq_prep(lg_ctx* h, const Plan& pl, int off, int n, hipStream_t s, hipEvent_t ev_prep) {
    h->export_pending = true;
    const size_t px = (size_t)pl.H * pl.W, words = (size_t)pl.H * pl.WW;
    LG_HIP(h, hipMemsetAsync(h->maxfix + LG_MF * (size_t)off, 0, sizeof(uint32_t) * LG_MF * n, s));
    if (pl.label_aware) LG_HIP(h, hipMemsetAsync(h->iso_mf + LG_ISO_MF * (size_t)off, 0, sizeof(uint32_t) * LG_ISO_MF * n, s));
    {
        ProfScope ps(h, "prep", s);
        if (pl.labels && pl.label_aware)   // (one sub-batch: off = 0)
            lg_launch_pack_labels(pl.labels + off * px, h->ids_dev + off, h->mask_ws + off * px, h->bits + off * words, n, pl.H, pl.W,
                                  pl.WW, s, h->maxfix + LG_MF * (size_t)off, h->iso_others + off * words, h->iso_mf + LG_ISO_MF * (size_t)off);
        else if (pl.labels)
            lg_launch_pack_labels(pl.labels + off * px, h->ids_dev + off, h->mask_ws + off * px, h->bits + off * words, n, pl.H, pl.W,
                                  pl.WW, s, h->maxfix + LG_MF * (size_t)off);
        else
            lg_launch_pack_bits(pl.mask + off * px, h->bits + off * words, n, pl.H, pl.W, pl.WW, s, h->maxfix + LG_MF * (size_t)off);
    }
    {
        ProfScope ps(h, "bbox", s);
        lg_launch_window(h->maxfix + LG_MF * (size_t)off, h->win + off, n, pl.H, pl.W, h->opt.dt_search, s);
    }
    LG_HIP(h, hipEventRecord(ev_prep, s));
    LG_HIP(h, hipStreamWaitEvent(h->copy_stream, ev_prep, 0));
    if (pl.near) {   // (one sub-batch: off = 0, n = B)  list offsets of the near tiles + the far tiles' keys and state bytes
        // On the caller's stream, which (the row search runs on a stream of its own) has little to do until the plane kernel and
        // orders the plane kernel and top-k behind it for free -- not in front of the orientation kernel on the side stream,
        // whose chain nothing of this feeds.  The host reads near_off_host[n] behind ev_near (enq_final), after ev_orient.
        ProfScope ps(h, "near_tiles", s);
        lg_launch_near_tiles(h->win, n, pl.H, pl.W, pl.P.gaussian_size / 2 + 1, h->near_off, h->near_off_host_dev, h->tilekeys,
                             h->tile_state, s);
        if (!h->near_off_host_dev)
            LG_HIP(h, hipMemcpyAsync(h->near_off_host, h->near_off, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, s));
        LG_HIP(h, hipEventRecord(h->ev_near, s));
    }
    if (h->orient) {   // contour analysis on the device, beside the sweeps; the host reads theta / status behind ev_orient
        // where the pinned copies have device aliases the kernel writes them itself, else they are copied back
        const bool direct = h->fp_host_dev && h->orient->h_status_dev;
        {
            ProfScope ps(h, "orient", h->copy_stream);
            lg_launch_orient(h->orient, h->bits + off * words, h->win + off, h->fp_dev + off, off, n, pl.H, pl.W, pl.WW, h->copy_stream,
                             direct ? h->fp_host_dev + off : nullptr);
        }
        if (!direct) {
            LG_HIP(h, hipMemcpyAsync(h->fp_host + off, h->fp_dev + off, sizeof(LgFrameParams) * n, hipMemcpyDeviceToHost, h->copy_stream));
            LG_HIP(h, hipMemcpyAsync(h->orient->h_status + off, h->orient->status + off, sizeof(int) * n, hipMemcpyDeviceToHost,
                                     h->copy_stream));
        }
        LG_HIP(h, hipEventRecord(h->ev_orient, h->copy_stream));
    }
    if (h->opt.side_tail) {   // beside the sweeps (latency bound, two workgroups per CU), not behind them: 0.3 ms per 256 frames;
        // LG_SIDE_TAIL=2 puts them on a third stream whatever the batch, so that orientation -> border -> stem is not one chain as
        // long as the sweeps themselves -- measured slower at 256 frames (9.76-9.94 vs 9.56-9.77 ms per step, three alternating runs;
        // again with form 5 of the search, whose chain is the shorter one: 2.196, 2.199 vs 2.135, 2.162 ms, NOTES_dt_bands; and
        // with the pruned border search and the two-level hull test, which make the side chain the shorter one again, 0.34 against
        // 0.45 ms: 2.074, 2.093 vs 2.044 .. 2.061 ms, NOTES_side_chain; and with form 6 of the search, one workgroup per CU: 2.070,
        // 2.047, 2.018 vs 2.004, 2.026, 2.011 ms -- the stem bits' dilation and the sweep share the vector ALUs, both take longer,
        // NOTES_dt_sweep; and with the nested-span stem kernel, 0.084 instead of 0.101 ms: 1.9005, 1.8853, 1.9201 vs 1.9185, 1.9067,
        // 1.8976 ms, not every run faster, NOTES_side_copies)
        // Small batches are a chain of latencies, not of throughput: orientation (0.13 ms for one frame; 0.10 since the two-level
        // hull test), border maxima (0.08; 0.035 since the pruned search) and stem bits (0.01) one behind the other on the side
        // stream were the longest chain between the bit rows and the plane kernel of a single-frame call (0.22 ms; the row search
        // beside them takes 0.10).  Up to 32 frames the border maxima and the stem bits go to a stream of their own (s_dt[0]; the
        // search uses s_dt[1]).
        const bool own_tail = h->opt.subbatch == 0 && (h->opt.side_tail == 2 || n <= 32);
        hipStream_t ts = own_tail ? h->s_dt[0] : h->copy_stream;
        if (ts != h->copy_stream) LG_HIP(h, hipStreamWaitEvent(ts, ev_prep, 0));
        const int rc = enq_tail(h, pl, off, n, ts);
        if (rc) return rc;
        LG_HIP(h, hipEventRecord(h->ev_side, ts));
    }
    return LG_OK;
}

// Bit rows of the bounding boxes + the windows to the host: only for the host contour analysis (LG_HOST_ORIENT, or frames the
// device orientation kernel hands back) -- since round 3 the pre-grasp probes run on the device (lg_finish_kernel) and a normal
// call exports nothing.  The export writes pinned host memory over PCIe and slows every memory-bound kernel beside it about 4x,
// which is why it is only queued when somebody is about to wait for it.  `after`: an event to wait for first, or nullptr.
int enq_export(lg_ctx* h, const Plan& pl, int off, int n, hipEvent_t after) {
    const size_t words = (size_t)pl.H * pl.WW;
    if (after) LG_HIP(h, hipStreamWaitEvent(h->copy_stream, after, 0));
    if (h->bits_host_dev)   // rows of the bounding boxes only, posted writes by a small grid on the priority stream
        lg_launch_export_rows(h->bits + off * words, h->win + off, h->bits_host_dev + off * words, n, pl.H, pl.WW, h->copy_stream);
    else
        LG_HIP(h, hipMemcpyAsync(h->bits_host + off * words, h->bits + off * words, sizeof(unsigned long long) * n * words,
                                 hipMemcpyDeviceToHost, h->copy_stream));
    LG_HIP(h, hipMemcpyAsync(h->win_host + off, h->win + off, sizeof(LgWin) * n, hipMemcpyDeviceToHost, h->copy_stream));
    LG_HIP(h, hipEventRecord(h->ev_copy, h->copy_stream));
    h->export_pending = false;
    return LG_OK;
}

// forward + backward distance sweeps (+ frame-border maxima and stem bits when they do not run on the side stream)
int enq_dt(lg_ctx* h, const Plan& pl, int off, int n, hipStream_t s) {
    const size_t px = (size_t)pl.H * pl.W, words = (size_t)pl.H * pl.WW;
    // d_in by the row search for the frames lg_window_kernel picked (LgWin::search_in), on a stream of its own beside the sweeps of
    // the other frames (and the d_out sweeps of the few frames that need them): throughput-bound work on every CU next to
    // latency-bound work on one workgroup per frame.  Inside the sub-batch pipeline (whose stages own the side streams): in line.
    hipStream_t ss = (s == h->s_dt[0] || s == h->s_dt[1]) ? s : h->s_dt[1];
    h->last_dt_algo = 0;
    h->last_iso_B = 0;   // (the sweeps' scratch held the fields of an earlier label-aware call)
    if (h->opt.dt_search) {
        if (ss != s) LG_HIP(h, hipStreamWaitEvent(ss, h->ev_prep, 0));
        {
            ProfScope ps(h, "dt_hrun", ss);
            lg_launch_hrun(h->bits + off * words, h->tmp + 2 * off * px, h->win + off, n, pl.H, pl.W, pl.WW, ss);
        }
        const int form = lg_dt_form(h->opt.dt_algo, n, pl.H, pl.W);
        h->last_dt_algo = form;
        const unsigned long long* bits = h->bits + off * words;
        uint32_t *tmp = h->tmp + 2 * off * px, *maxfix = h->maxfix + LG_MF * (size_t)off;
        float* dist = pl.maps[LG_MAP_DISTANCE] + off * px;
        const LgWin* win = h->win + off;
        {
            ProfScope ps(h, "dt_search", ss);   // the one-level search, the seed rows, or the whole box by the register sweep
            switch (form) {
                case LG_DT_FORM_BANDS: lg_launch_dt_seeds(bits, tmp, dist, maxfix, win, n, pl.H, pl.W, pl.WW, h->opt.dt_band_p, ss); break;
                case LG_DT_FORM_SWEEP: lg_launch_dt_sweep(tmp, dist, maxfix, win, n, pl.H, pl.W, ss); break;
                default: lg_launch_dt_rows(bits, tmp, dist, maxfix, win, n, pl.H, pl.W, pl.WW, ss); break;
            }
        }
        if (form == LG_DT_FORM_BANDS) {
            ProfScope ps(h, "dt_band", ss);     // the rows between the seed pairs
            lg_launch_dt_bands(bits, tmp, dist, maxfix, win, n, pl.H, pl.W, pl.WW, h->opt.dt_band_p, h->opt.dt_band_e, ss);
        }
        if (ss != s) LG_HIP(h, hipEventRecord(h->ev_search, ss));
    }
    {
        ProfScope ps(h, "dt_fwd", s);
        if (lg_launch_dt(false, pl.mask + off * px, h->tmp + 2 * off * px, nullptr, h->maxfix + LG_MF * (size_t)off, h->win + off, n,
                         pl.H, pl.W, (uint32_t)pl.P.chamfer_init_dist0, s))
            return fail(h, LG_ERR_UNSUPPORTED, "dt: width");
    }
    {
        ProfScope ps(h, "dt_bwd", s);
        lg_launch_dt(true, pl.mask + off * px, h->tmp + 2 * off * px, pl.maps[LG_MAP_DISTANCE] + off * px,
                     h->maxfix + LG_MF * (size_t)off, h->win + off, n, pl.H, pl.W, (uint32_t)pl.P.chamfer_init_dist0, s);
    }
    if (h->opt.dt_search && ss != s) LG_HIP(h, hipStreamWaitEvent(s, h->ev_search, 0));
    if (!h->opt.side_tail) return enq_tail(h, pl, off, n, s);
    return LG_OK;
}

// host contour analysis of one frame (its bit rows must have landed: ev_copy synchronised)
void host_orient_frame(lg_ctx* h, const Plan& pl, int b) {
    const int H = pl.H, W = pl.W, WW = pl.WW;
    double o[5];
    // only the rows / words of the bounding box are on the host: analyse them as a band (the rest is all zero)
    const LgWin& w = h->win_host[b];
    const int hy = w.by1 - w.by0 + 1;
    int ok = hy > 0 ? lg_host_orientation_band(h->bits_host + ((size_t)b * H + w.by0) * WW, hy, W, WW, w.by0, w.bx0 >> 6, w.bx1 >> 6, o) : 0;
    LgFrameParams f;
    f.has_angle = ok;
    f.theta = ok ? (float)o[0] : NAN;
    f.sin_t = ok ? (float)sin(o[0]) : 0.f;
    f.cos_t = ok ? (float)cos(o[0]) : 0.f;
    h->fp_host[b] = f;
}

// Orientation of frames [off, off+n) into fp_host (and fp_dev).  Device path: wait for lg_orient_kernel's results (it runs
// beside the sweeps on the side stream); frames it handed back (status 1: more runs than its scratch holds) are analysed on
// the host threads.  LG_HOST_ORIENT: every frame on the host.  *upload = fp_host has entries the device does not have yet.
int finish_orient(lg_ctx* h, const Plan& pl, int off, int n, bool* upload) {
    *upload = true;
    h->last_redo = 0;
    if (!h->orient) {
        if (h->export_pending) { const int rc = enq_export(h, pl, 0, pl.B, nullptr); if (rc) return rc; }
        LG_HIP(h, hipEventSynchronize(h->ev_copy));   // bit rows are on the host; the sweeps are running
        parallel_for(h, n, [=, &pl](int i) { host_orient_frame(h, pl, off + i); });
        return LG_OK;
    }
    LG_HIP(h, hipEventSynchronize(h->ev_orient));
    std::vector<int> redo;
    for (int i = 0; i < n; i++)
        if (h->orient->h_status[off + i]) redo.push_back(off + i);
    h->last_redo = (int)redo.size();
    *upload = !redo.empty();
    if (redo.empty()) return LG_OK;
    if (h->export_pending) { const int rc = enq_export(h, pl, 0, pl.B, nullptr); if (rc) return rc; }
    LG_HIP(h, hipEventSynchronize(h->ev_copy));
    const int* rp = redo.data();
    parallel_for(h, (int)redo.size(), [=, &pl](int i) { host_orient_frame(h, pl, rp[i]); });
    return LG_OK;
}

// frame scalars H2D + the fused score-plane kernel
int enq_final(lg_ctx* h, const Plan& pl, int off, int n, hipStream_t s, bool upload_fp, LgFinalArgs* keep = nullptr) {
    const size_t px = (size_t)pl.H * pl.W, words = (size_t)pl.H * pl.WW;
    const int H = pl.H, W = pl.W;
    const lg_params& P = pl.P;
    if (h->orient) LG_HIP(h, hipStreamWaitEvent(s, h->ev_orient, 0));   // fp_dev was written on the side stream
    if (h->opt.side_tail) LG_HIP(h, hipStreamWaitEvent(s, h->ev_side, 0));  // maxfix (d_out border) and the stem bits
    if (upload_fp) LG_HIP(h, hipMemcpyAsync(h->fp_dev + off, h->fp_host + off, sizeof(LgFrameParams) * n, hipMemcpyHostToDevice, s));
    LgFinalArgs a;
    memset(&a, 0, sizeof(a));
    a.depth = pl.depth + off * px; a.bits = h->bits + off * words; a.stem_bits = h->stem + off * words;
    a.maxfix = h->maxfix + LG_MF * (size_t)off; a.fp = h->fp_dev + off;
    a.win = h->win + off; a.win_wc = lg_dt_geometry(W, nullptr);
    for (int i = 0; i < LG_NUM_MAPS; i++) a.maps[i] = pl.maps[i] ? pl.maps[i] + off * px : nullptr;
    a.valid = pl.valid ? pl.valid + off * px : nullptr;
    a.tilekeys = h->tilekeys + (size_t)off * pl.tiles_x * pl.tiles_y;
    a.tile_state = pl.sparse ? h->tile_state + (size_t)off * pl.tiles_x * pl.tiles_y : nullptr;
    a.sparse = pl.sparse ? 1 : 0;
    a.score_only = pl.defer ? 1 : 0;
    a.B = n; a.H = H; a.W = W; a.WW = pl.WW; a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y;
    a.cxi = (int)floor(P.cx); a.cyi = (int)floor(P.cy);
    a.cxf = (float)(P.cx - floor(P.cx)); a.cyf = (float)(P.cy - floor(P.cy)); a.f = (float)P.f;
    a.w_approach = P.w_approach; a.w_sdf = P.w_sdf; a.w_flat = P.w_flat; a.w_access = P.w_access;
    a.sdf_w_interior = P.sdf_w_interior; a.sdf_w_align = P.sdf_w_align; a.sdf_w_sdf = P.sdf_w_sdf;
    a.optimal_distance = P.optimal_distance;
    a.access_w_dist = P.access_w_dist; a.access_w_dir = P.access_w_dir; a.flat_scale = P.flat_scale;
    a.iso_w_close = P.iso_w_close; a.iso_w_wide = P.iso_w_wide;
    a.iso_ramp_top = P.iso_ramp_top; a.iso_ramp_bottom = P.iso_ramp_bottom;
    {
        // max of the chamfer-3 transform of an all-ones image: INIT + ceil(min(H,W)/2) * 0.955
        uint32_t dmax = (uint32_t)((std::min(H, W) + 1) / 2);
        float mx = (float)((uint32_t)P.chamfer_init_dist0 + dmax * LG_A3) * (1.0f / 65536.0f);
        a.init0 = (uint32_t)P.chamfer_init_dist0;
        a.iso_inv_max = 1.0f / mx;  // reference divides by (max + 1e-6), which rounds to max in float32
    }
    a.min_edge_distance = P.min_edge_distance; a.stem_valid_thresh = P.stem_valid_thresh;
    a.inv_maxd = (float)(1.0 / sqrt((double)W * W + (double)H * H));
    a.inv_2s2 = 1.0f / (2.0f * P.optimal_distance * P.optimal_distance);   // (correctly rounded, like the device's __frcp_rn)
    a.iso_ramp_step = (H > 1) ? (P.iso_ramp_bottom - P.iso_ramp_top) / (float)(H - 1) : 0.0f;
    gaussian1d(P.gaussian_size, a.k1);
    a.gauss_r = P.gaussian_size / 2;
    a.no_skip = h->opt.no_skip;
    a.persist = h->opt.final_persist;   // (lg_launch_final: the tile walk and the tiles per workgroup stay experiment switches)
    a.tpw = h->opt.final_tpw;
    a.nt_stores = 0;
    if (pl.near) {   // (one sub-batch: off = 0, n = B)
        LG_HIP(h, hipEventSynchronize(h->ev_near));   // near_off_host is written (the kernel ended long ago: it follows the bit-row pass)
        a.near_off = h->near_off;
        a.near_total = h->near_off_host[n];
        a.near_tpw = h->opt.final_near;
    }
    {
        ProfScope ps(h, "final", s, true);
        lg_launch_final(a, s, ps.slot ? ps.e0 : nullptr, ps.slot ? ps.e1 : nullptr);
    }
    if (keep) *keep = a;   // (the deferred gather of these frames runs the same per-pixel code on the same arguments)
    return LG_OK;
}

int make_plan(lg_ctx* h, Plan& pl, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
              float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, const char* who) {
    if (!depth || !mask || B <= 0 || H < 8 || W < 8 || W > 8192 || H > 16384)
        return fail(h, LG_ERR_INVALID, "bad pointer or shape (need H,W >= 8, W <= 8192)");
    if (pin) pl.P = *pin; else lg_default_params(&pl.P);
    if (pl.P.stem_se < 1 || pl.P.stem_se > 64 || pl.P.stem_bottom_div < 1)
        return fail(h, LG_ERR_INVALID, "stem_se must be in [1,64], stem_bottom_div >= 1");
    if (pl.P.nms_min_distance < 0 || pl.P.pregrasp_clearance < 0 || pl.P.pregrasp_clearance > 31)
        return fail(h, LG_ERR_INVALID, "nms_min_distance must be >= 0, pregrasp_clearance in [0,31]");
    // _calculate_flatness_map smooths with the caller's ImageProcessor (grasp_point_selector.py:635-657): an even size gives
    // an (H+1) x (W+1) plane there and the fusion raises -> None triple; odd sizes above 7 exceed this kernel's halo
    if (pl.P.gaussian_size < 1 || pl.P.gaussian_size > 7 || (pl.P.gaussian_size & 1) == 0)
        return fail(h, LG_ERR_UNSUPPORTED, "gaussian_size must be 1, 3, 5 or 7 (an even size fails in the reference too: shape mismatch in the fusion)");
    if (pl.P.gaussian_size / 2 >= std::min(H, W))   // torch's reflect padding refuses it: the reference ends in its None triple
        return fail(h, LG_ERR_INVALID, "gaussian_size / 2 must be smaller than H and W (reflect padding)");
    if (pl.P.chamfer_init_dist0 < (int32_t)LG_INIT0)   // (a zeroed struct, or a value a real distance could reach)
        return fail(h, LG_ERR_INVALID, "chamfer_init_dist0 must be in [INT_MAX >> 2, INT_MAX] (lg_default_params: INT_MAX >> 2)");
    if (lg_label_aware_check(&pl.P, 1)) return fail(h, LG_ERR_INVALID, "label_aware must be 0 or 1");
    pl.B = B; pl.H = H; pl.W = W; pl.WW = (W + 63) / 64;
    pl.tiles_x = (W + LG_TW - 1) / LG_TW; pl.tiles_y = (H + LG_TH - 1) / LG_TH;
    if (pl.tiles_x * pl.tiles_y > 8192) return fail(h, LG_ERR_UNSUPPORTED, "image too large for the top-k tile table");
    pl.depth = depth; pl.mask = mask; pl.valid = out_valid;
    for (int i = 0; i < LG_NUM_MAPS; i++) pl.maps[i] = out_maps ? out_maps[i] : nullptr;
    (void)who;
    return LG_OK;
}

}  // namespace

extern "C" {

int lg_score_maps(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                  float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, float* theta_host, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, out_maps, out_valid, "lg_score_maps");
    if (rc) return rc;
    if (lg_label_aware_check(&pl.P, 0)) return fail(h, LG_ERR_INVALID, "lg_score_maps: label_aware needs the label image (lg_select_grasp_labels, lg_select_grasp_candidates_labels)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    rc = ensure_ws(h, B, H, W, pl.P.top_k);
    if (rc) return rc;
    for (int i : {LG_MAP_DISTANCE, LG_MAP_TRADITIONAL})
        if (!pl.maps[i]) {
            rc = ensure_ws_map(h, i);
            if (rc) return rc;
            pl.maps[i] = h->ws_maps[i];
        }
    if (!pl.valid) pl.valid = h->ws_valid;
    rc = enq_prep(h, pl, 0, B, s, h->ev_prep);
    if (rc) return rc;
    rc = enq_dt(h, pl, 0, B, s);
    if (rc) return rc;
    // ---- orientation: lg_orient_kernel beside the distance-transform sweeps (host threads for frames it hands back)
    bool upload_fp = true;
    rc = finish_orient(h, pl, 0, B, &upload_fp);
    if (rc) return rc;
    if (theta_host)
        for (int b = 0; b < B; b++) theta_host[b] = h->fp_host[b].theta;
    rc = enq_final(h, pl, 0, B, s, upload_fp);
    if (rc) return rc;
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_smooth_depth(lg_handle h, const float* depth, int B, int H, int W, int gaussian_size, float* out, void* stream_) {
    // Stateless: only the handle's device is read, nothing of the handle is written -- the Python ImageProcessor objects of a
    // process share one handle per device across threads, so this entry point takes no part in the one-call-in-flight rule and
    // leaves the handle's error string alone (the reason of a failure: lg_last_error(NULL), per thread).
    if (!h) return LG_ERR_INVALID;
    auto bad = [](int code, const char* what) { g_create_err = what; return code; };
    if (!depth || !out || B < 1 || H < 1 || W < 1) return bad(LG_ERR_INVALID, "lg_smooth_depth: bad argument");
    if (gaussian_size < 1 || gaussian_size > LG_MAX_GAUSS) return bad(LG_ERR_UNSUPPORTED, "lg_smooth_depth: gaussian_size must be in [1,15]");
    if (gaussian_size / 2 >= std::min(H, W))   // torch: "Padding size should be less than the corresponding input dimension"
        return bad(LG_ERR_INVALID, "lg_smooth_depth: reflect padding (gaussian_size / 2) must be smaller than H and W");
    if (hipSetDevice(h->device) != hipSuccess) return bad(LG_ERR_HIP, "lg_smooth_depth: hipSetDevice failed");
    LgGaussTaps taps;
    memset(&taps, 0, sizeof(taps));
    gaussian1d(gaussian_size, taps.k);
    lg_launch_smooth(depth, out, B, H, W, gaussian_size, taps, (hipStream_t)stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_create_err = std::string("lg_smooth_depth: ") + hipGetErrorString(e); return LG_ERR_HIP; }
    return LG_OK;
}

int lg_gaussian_taps(int gaussian_size, float* taps) {
    if (!taps || gaussian_size < 1 || gaussian_size > LG_MAX_GAUSS) return LG_ERR_INVALID;
    gaussian1d(gaussian_size, taps);
    return LG_OK;
}

int lg_topk_nms(lg_handle h, const float* trad, const uint8_t* valid, int B, int H, int W, int k, int min_dist,
                int32_t* out_xy, int32_t* out_n, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!trad || !valid || !out_xy || !out_n || B <= 0 || H < 1 || W < 1 || k < 1 || k > 64 || min_dist < 0)
        return fail(h, LG_ERR_INVALID, "lg_topk_nms: bad argument (1 <= k <= 64)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    const int tiles = ((W + LG_TW - 1) / LG_TW) * ((H + LG_TH - 1) / LG_TH);
    if (tiles > 8192) return fail(h, LG_ERR_UNSUPPORTED, "lg_topk_nms: image too large");
    int rc = ensure_ws(h, B, H, W, k);
    if (rc) return rc;
    ProfScope ps(h, "topk", s);
    lg_launch_topk(trad, valid, nullptr, h->tilekeys, nullptr, 0.0f, 0.0f, false, B, H, W, k, min_dist, out_xy, out_n, nullptr, s);
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_gather_patches(lg_handle h, const float* depth, const uint8_t* mask, const float* const maps[LG_NUM_MAPS], int B,
                      int H, int W, int k, const int32_t* xy, const int32_t* n, float* patches, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!depth || !mask || !maps || !xy || !n || !patches || B <= 0 || k < 1)
        return fail(h, LG_ERR_INVALID, "lg_gather_patches: bad argument");
    for (int i = 0; i < 7; i++)
        if (!maps[i]) return fail(h, LG_ERR_INVALID, "lg_gather_patches: maps[0..6] are required");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    ProfScope ps(h, "gather", s);
    lg_launch_gather(depth, mask, maps, nullptr, 0.0f, B, H, W, k, xy, n, patches, false, s);
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_harvest_patches(lg_handle h, const float* depth, const uint8_t* mask, const float* const maps[LG_NUM_MAPS], int H,
                       int W, int n, const int32_t* xy, const int32_t* rot, float* out_depth, float* out_mask,
                       float* out_scores, int32_t* flags, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!depth || !mask || !maps || !xy || !out_depth || !out_mask || !out_scores || !flags || n < 1 || H < 32 || W < 32)
        return fail(h, LG_ERR_INVALID, "lg_harvest_patches: bad argument");
    for (int i = 0; i < 7; i++)
        if (!maps[i]) return fail(h, LG_ERR_INVALID, "lg_harvest_patches: maps[0..6] are required");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    lg_launch_harvest(depth, mask, maps, H, W, n, xy, rot, out_depth, out_mask, out_scores, flags, s);
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_negative_masks(lg_handle h, const float* distance_map, const uint8_t* mask, int H, int W, uint8_t* out_tip,
                      uint8_t* out_stem, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!distance_map || !mask || !out_tip || !out_stem || H < 1 || W < 1)
        return fail(h, LG_ERR_INVALID, "lg_negative_masks: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1, H, W, 20);
    if (rc) return rc;
    // scratch for the first erosion: the u8 view of the forward-sweep workspace (H*W bytes needed, 8*H*W available)
    h->last_iso_B = 0;
    lg_launch_negative_masks(distance_map, mask, out_tip, out_stem, reinterpret_cast<uint8_t*>(h->tmp), H, W, s);
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_leaf_contour(lg_handle h, const uint8_t* mask, int H, int W, int32_t* out_xy, int cap, int* n_out, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!mask || !n_out || (cap > 0 && !out_xy) || cap < 0 || H < 1 || W < 1)
        return fail(h, LG_ERR_INVALID, "lg_leaf_contour: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1, H, W, 20);
    if (rc) return rc;
    const int WW = (W + 63) / 64;
    lg_launch_pack_bits(mask, h->bits, 1, H, W, WW, s);
    LG_HIP(h, hipMemcpyAsync(h->bits_host, h->bits, sizeof(unsigned long long) * (size_t)H * WW, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    std::vector<int> pts;
    const int n = lg_host_contour_points(h->bits_host, H, W, WW, pts);
    *n_out = n;
    for (int i = 0; i < n && i < cap; i++) { out_xy[2 * i] = pts[2 * i]; out_xy[2 * i + 1] = pts[2 * i + 1]; }
    return LG_OK;
}

int lg_leaf_orientation(lg_handle h, const uint8_t* mask, int H, int W, float* out, int* found, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!mask || !out || !found || H < 1 || W < 1) return fail(h, LG_ERR_INVALID, "lg_leaf_orientation: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    int rc = ensure_ws(h, 1, H, W, 20);
    if (rc) return rc;
    const int WW = (W + 63) / 64;
    LG_HIP(h, hipMemsetAsync(h->maxfix, 0, sizeof(uint32_t) * LG_MF, s));   // (the bounding box accumulates from zero)
    lg_launch_pack_bits(mask, h->bits, 1, H, W, WW, s, h->maxfix);
    double o[5];
    if (h->orient) {   // the device analysis; a mask with more runs than its scratch holds falls through to the host code
        lg_launch_window(h->maxfix, h->win, 1, H, W, 0, s);
        lg_launch_orient(h->orient, h->bits, h->win, h->fp_dev, 0, 1, H, W, WW, s);
        LG_HIP(h, hipMemcpyAsync(h->orient->h_out, h->orient->out, sizeof(double) * 5, hipMemcpyDeviceToHost, s));
        LG_HIP(h, hipMemcpyAsync(h->orient->h_status, h->orient->status, sizeof(int), hipMemcpyDeviceToHost, s));
        LG_HIP(h, hipStreamSynchronize(s));
        if (!h->orient->h_status[0]) {
            *found = !std::isnan(h->orient->h_out[0]);
            for (int i = 0; i < 5; i++) out[i] = *found ? (float)h->orient->h_out[i] : NAN;
            return LG_OK;
        }
    }
    LG_HIP(h, hipMemcpyAsync(h->bits_host, h->bits, sizeof(unsigned long long) * (size_t)H * WW, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    *found = lg_host_orientation(h->bits_host, H, W, WW, o);
    for (int i = 0; i < 5; i++) out[i] = *found ? (float)o[i] : NAN;
    return LG_OK;
}

int lg_clahe(lg_handle h, const uint8_t* src, int B, int H, int W, double clip_limit, int tiles_x, int tiles_y, uint8_t* dst,
             void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    LgClaheGeom g;
    if (!src || !dst || B < 1 || lg_clahe_geom(H, W, clip_limit, tiles_x, tiles_y, &g))
        return fail(h, LG_ERR_INVALID, "lg_clahe: bad argument (tiles 1..64 each, H, W >= 2)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    const int ntiles = tiles_x * tiles_y;
    std::string err;
    if (lg_midrib_ensure(h->midrib, B, H, W, ntiles, false, false, h->opt.orient_cap, &err)) return fail(h, LG_ERR_NOMEM, err.c_str());
    LG_HIP(h, hipMemsetAsync(h->midrib->hist, 0, sizeof(int) * (size_t)B * ntiles * 256, s));
    {
        ProfScope ps(h, "clahe_hist", s);
        lg_launch_clahe_hist(src, nullptr, 0, B, g, h->midrib->hist, s);
    }
    {
        ProfScope ps(h, "clahe_lut", s);
        lg_launch_clahe_lut(h->midrib->hist, h->midrib->lut, B, g, s);
    }
    {
        ProfScope ps(h, "clahe_apply", s);
        lg_launch_clahe_apply(src, h->midrib->lut, B, g, dst, s);
    }
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_detect_midrib(lg_handle h, const uint8_t* image, int C, const uint8_t* mask, int B, int H, int W, int32_t* out,
                     int32_t* status, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    LgClaheGeom g;
    if (!image || !mask || !out || !status || B < 1 || (C != 3 && C != 4) || lg_clahe_geom(H, W, 3.0, 8, 8, &g))
        return fail(h, LG_ERR_INVALID, "lg_detect_midrib: bad argument (C 3 or 4, H, W >= 2)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    const int ntiles = 64, WW = (W + 63) / 64;
    std::string err;
    const bool dev_orient = !h->opt.host_orient && H <= 16384 && W <= 8192;   // lg_leaf_orientation's condition (ensure_ws)
    if (lg_midrib_ensure(h->midrib, B, H, W, ntiles, true, dev_orient, h->opt.orient_cap, &err)) return fail(h, LG_ERR_NOMEM, err.c_str());
    LgMidribWs* m = h->midrib;
    // CLAHE(clipLimit=3.0, tileGridSize=(8,8)) of the masked gray (:834-843): histograms and LUTs; the enhanced image itself is
    // evaluated by the walk at its samples only
    LG_HIP(h, hipMemsetAsync(m->hist, 0, sizeof(int) * (size_t)B * ntiles * 256, s));
    {
        ProfScope ps(h, "midrib_hist", s);
        lg_launch_clahe_hist(image, mask, C, B, g, m->hist, s);
    }
    {
        ProfScope ps(h, "midrib_lut", s);
        lg_launch_clahe_lut(m->hist, m->lut, B, g, s);
    }
    // estimate_leaf_orientation (:858) of every frame, as lg_leaf_orientation computes it
    {
        ProfScope ps(h, "midrib_orient", s);
        if (m->orient) LG_HIP(h, hipMemsetAsync(m->box, 0, sizeof(uint32_t) * LG_MF * B, s));
        lg_launch_pack_bits(mask, m->bits, B, H, W, WW, s, m->orient ? m->box : nullptr);
        if (m->orient) {
            lg_launch_window(m->box, m->win, B, H, W, 0, s);
            lg_launch_orient(m->orient, m->bits, m->win, m->fp, 0, B, H, W, WW, s);
            LG_HIP(h, hipMemcpyAsync(m->orient->h_out, m->orient->out, sizeof(double) * 5 * B, hipMemcpyDeviceToHost, s));
            LG_HIP(h, hipMemcpyAsync(m->orient->h_status, m->orient->status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        }
    }
    LG_HIP(h, hipStreamSynchronize(s));
    bool host_needed = !m->orient;
    for (int b = 0; b < B && !host_needed; b++) host_needed = m->orient->h_status[b] != 0;
    if (host_needed) {
        LG_HIP(h, hipMemcpyAsync(m->bits_host, m->bits, sizeof(unsigned long long) * (size_t)B * H * WW, hipMemcpyDeviceToHost, s));
        LG_HIP(h, hipStreamSynchronize(s));
    }
    for (int b = 0; b < B; b++) {
        float o[5];
        int found;
        if (m->orient && !m->orient->h_status[b]) {
            const double* d = m->orient->h_out + 5 * (size_t)b;
            found = !std::isnan(d[0]);
            for (int i = 0; i < 5; i++) o[i] = (float)d[i];
        } else {
            double d[5];
            found = lg_host_orientation(m->bits_host + (size_t)b * H * WW, H, W, WW, d);
            for (int i = 0; i < 5; i++) o[i] = (float)d[i];
        }
        lg_midrib_setup(found, o, &m->geom_host[b]);
    }
    LG_HIP(h, hipMemcpyAsync(m->geom, m->geom_host, sizeof(LgMidribGeom) * B, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(h, "midrib_walk", s);
        lg_launch_midrib_walk(image, C, mask, m->lut, B, g, m->geom, m->res, s);
    }
    LG_HIP(h, hipGetLastError());
    LG_HIP(h, hipMemcpyAsync(m->res_host, m->res, sizeof(int32_t) * 5 * B, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        for (int i = 0; i < 4; i++) out[4 * (size_t)b + i] = m->res_host[5 * (size_t)b + i];
        status[b] = m->res_host[5 * (size_t)b + 4];
    }
    return LG_OK;
}

int lg_leaf_stats(lg_handle h, const int16_t* labels, const float* depth, int H, int W, float cx, float cy, float f,
                  lg_leaf_stat* stats, int max_leaves, int* n_leaves, int32_t* extrema, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!labels || !depth || !stats || !n_leaves || !extrema || H < 1 || W < 1 || max_leaves < 1)
        return fail(h, LG_ERR_INVALID, "lg_leaf_stats: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    std::string err;
    ProfScope ps(h, "leaf", s);
    int rc = lg_leaf_run(h->leaf, labels, depth, H, W, cx, cy, f, stats, max_leaves, n_leaves, extrema, s, h->s_dt[0], &err, h->leaf_prof);
    if (rc) return fail(h, rc, err.c_str());
    return LG_OK;
}

int lg_leaf_stats_batch(lg_handle h, const int16_t* labels, const float* depth, int B, int H, int W, float cx, float cy,
                        float f, lg_leaf_stat* stats, int max_leaves, int* n_leaves, int32_t* extrema, int* status,
                        void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!labels || !depth || !stats || !n_leaves || !extrema || !status || B < 1 || H < 1 || W < 1 || max_leaves < 1)
        return fail(h, LG_ERR_INVALID, "lg_leaf_stats_batch: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    std::string err;
    ProfScope ps(h, "leaf", s);
    int rc = lg_leaf_run_batch(h->leaf, labels, depth, B, H, W, cx, cy, f, stats, max_leaves, n_leaves, extrema, status, s,
                               h->s_dt[0], &err, h->leaf_prof);
    if (rc) return fail(h, rc, err.c_str());
    return LG_OK;
}

int lg_leaf_select_batch(lg_handle h, const int16_t* labels, const float* depth, int B, int H, int W, double cx, double cy,
                         double f, int32_t* ids, int32_t* n_tall, int32_t* tall, int tall_cap, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!labels || !depth || !ids || !n_tall || !tall || B < 1 || H < 1 || W < 1 || tall_cap < 1)
        return fail(h, LG_ERR_INVALID, "lg_leaf_select_batch: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    std::string err;
    ProfScope ps(h, "leaf", s);
    int rc;
    try {   // (the host half allocates: nothing may throw across the C boundary)
        rc = lg_leaf_select_batch_run(h->leaf, labels, depth, B, H, W, cx, cy, f, ids, n_tall, tall, tall_cap, s, h->s_dt[0], &err, h->leaf_prof);
    } catch (const std::bad_alloc&) {
        return fail(h, LG_ERR_NOMEM, "lg_leaf_select_batch: out of host memory");
    } catch (...) {
        return fail(h, LG_ERR_INVALID, "lg_leaf_select_batch: unexpected exception");
    }
    if (rc) return fail(h, rc, err.c_str());
    return LG_OK;
}

int lg_leaf_select_from_stats(const lg_leaf_stat* stats, int n, const int32_t* extrema, int H, int W, double cx, double cy, double f,
                              int32_t* id, int32_t* tall, int tall_cap, int32_t* n_tall) {
    if (!stats || !extrema || !id || !tall || !n_tall || n < 0 || H < 1 || W < 1 || tall_cap < 1) return LG_ERR_INVALID;
    int nt = 0;
    try {
        *id = lg_leaf_select_host(stats, n, extrema, H, W, cx, cy, f, tall, tall_cap, &nt);
    } catch (const std::bad_alloc&) {
        return LG_ERR_NOMEM;
    } catch (...) {
        return LG_ERR_INVALID;
    }
    *n_tall = nt;
    return LG_OK;
}

int lg_cnn_load(lg_handle h, const lg_cnn_weights* w) {
    if (!h || !w) return LG_ERR_INVALID;
    LG_ENTER(h);
    LG_HIP(h, hipSetDevice(h->device));
    std::string err;
    int rc = lg_cnn_upload(&h->cnn, w, &err);
    if (rc) return fail(h, rc, err.c_str());
    return LG_OK;
}

int lg_cnn_unload(lg_handle h) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    lg_cnn_free(&h->cnn);
    return LG_OK;
}

int lg_cnn_forward(lg_handle h, const float* patches, int N, float* logits, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!patches || !logits || N <= 0) return fail(h, LG_ERR_INVALID, "lg_cnn_forward: bad argument");
    if (!h->cnn.loaded) return fail(h, LG_ERR_NO_MODEL, "lg_cnn_forward: no model loaded (reference: ml_predictor is None)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    std::string err;
    if (lg_cnn_take_error(&h->cnn)) return fail(h, LG_ERR_HIP, "lg_cnn_forward: a split item of the previous forward did not receive its parts");
    ProfScope ps(h, "cnn", s);
    int rc = lg_cnn_run(&h->cnn, patches, false, N, logits, s, &err);
    if (rc) return fail(h, rc, err.c_str());
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

// The trainer's weights into this handle's inference CNN without leaving the device (lg_cnn_load.hip: the fold and transform kernels).
// The fold runs on the legacy default stream -- ordered after every blocking stream's earlier work, a forward on torch's default
// stream included -- behind an event recorded on each of the trainer's (non-blocking) streams.
int lg_cnn_load_from_trainer(lg_handle h, lg_trainer* t) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    LgTrainView v;
    if (!t || !lg_train_view(t, &v)) return fail(h, LG_ERR_INVALID, "lg_cnn_load_from_trainer: null trainer");
    if (v.device != h->device) return fail(h, LG_ERR_INVALID, "lg_cnn_load_from_trainer: the trainer lives on another device than the handle");
    LG_HIP(h, hipSetDevice(h->device));
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    LG_HIP(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (hipStream_t q : v.stream) {
        if (!q) continue;
        hipError_t e = hipEventRecord(ev, q);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
        if (e != hipSuccess) { hipEventDestroy(ev); return fail(h, LG_ERR_HIP, "lg_cnn_load_from_trainer: event", e); }
    }
    std::string err;
    const int rc = lg_cnn_upload_from_trainer(&h->cnn, &v, s, &err);   // synchronises s
    hipEventDestroy(ev);
    if (rc) return fail(h, rc, err.c_str());
    return LG_OK;
}

int lg_debug_cnn_weights(lg_handle h, int which, int layer, float* out, int64_t cap, int64_t* n) {
    if (!h || !n || cap < 0 || (cap > 0 && !out)) return LG_ERR_INVALID;
    LG_ENTER(h);
    *n = 0;
    const LgCnn& c = h->cnn;
    if (which == LG_CNNW_ALLOCS) { *n = (int64_t)c.weight_allocs; return LG_OK; }
    if (!c.loaded) return fail(h, LG_ERR_NO_MODEL, "lg_debug_cnn_weights: no model loaded");
    if (which == LG_CNNW_SCALARS) {
        std::vector<float> sc = {(float)c.n_layers, (float)c.F, (float)c.Fp, (float)c.npix, (float)c.act_per_patch, c.standard ? 1.f : 0.f,
                                 (float)c.att_type, c.att_type == LG_ATT_SPATIAL || c.att_type == LG_ATT_HYBRID ? c.att_b : 0.f};
        for (int L = 0; L < c.n_layers; L++) {
            const RtLayer& l = c.layers[L];
            for (int x : {l.cin, l.cout, l.cinp, l.coutp, l.wi, l.pool ? 1 : 0}) sc.push_back((float)x);
        }
        *n = (int64_t)sc.size();
        if (cap == 0) return LG_OK;
        if (cap < *n) return fail(h, LG_ERR_INVALID, "lg_debug_cnn_weights: cap too small");
        memcpy(out, sc.data(), sc.size() * sizeof(float));
        return LG_OK;
    }
    const float* p = nullptr;
    size_t cnt = 0;
    if (!lg_cnn_weight_buffer(&c, which, layer, &p, &cnt)) return LG_OK;   // no such buffer for this model: *n = 0
    *n = (int64_t)cnt;
    if (cap == 0) return LG_OK;   // size query
    if ((size_t)cap < cnt) return fail(h, LG_ERR_INVALID, "lg_debug_cnn_weights: cap too small");
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (hipMemcpy(out, p, cnt * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, LG_ERR_HIP, "lg_debug_cnn_weights: copy failed");
    return LG_OK;
}

// scratch of the metrics kernels (+ extra bytes behind it), grown when a call needs more
static int eval_scratch(lg_handle h, size_t bytes, hipStream_t s) {
    if (bytes <= h->eval_cap) return LG_OK;
    LG_HIP(h, hipStreamSynchronize(s));
    if (h->eval_ws) { hipFree(h->eval_ws); h->eval_ws = nullptr; h->eval_cap = 0; }
    if (hipMalloc(&h->eval_ws, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(h, LG_ERR_NOMEM, "lg_eval_logits: scratch allocation failed"); }
    h->eval_cap = bytes;
    return LG_OK;
}

static int eval_run(lg_handle h, const float* logits, const float* labels, int N, int chunk, double pos_weight, float threshold,
                    lg_eval_result* out, hipStream_t s) {
    lg_eval_enqueue(logits, labels, N, chunk, pos_weight, threshold, h->eval_ws, s);
    LG_HIP(h, hipGetLastError());
    lg_eval_result r;
    LG_HIP(h, hipMemcpyAsync(&r, h->eval_ws, sizeof(r), hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    *out = r;
    return LG_OK;
}

int lg_eval_logits(lg_handle h, const float* logits, const float* labels, int N, int chunk, double pos_weight, float threshold,
                   lg_eval_result* out, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!logits || !labels || !out || N < 1 || chunk < 1) return fail(h, LG_ERR_INVALID, "lg_eval_logits: bad argument");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    int rc = eval_scratch(h, lg_eval_scratch_bytes(N, chunk), s);
    if (rc) return rc;
    return eval_run(h, logits, labels, N, chunk, pos_weight, threshold, out, s);
}

// lg_cnn_forward's call of lg_cnn_run (same plan, same slices: the same logits) and the metrics behind it on the same stream
int lg_cnn_evaluate(lg_handle h, const float* patches, const float* labels, int N, int chunk, double pos_weight, float threshold,
                    float* logits_out, lg_eval_result* out, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!patches || !labels || !out || N < 1 || chunk < 1) return fail(h, LG_ERR_INVALID, "lg_cnn_evaluate: bad argument");
    if (!h->cnn.loaded) return fail(h, LG_ERR_NO_MODEL, "lg_cnn_evaluate: no model loaded (reference: ml_predictor is None)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    const size_t sb = (lg_eval_scratch_bytes(N, chunk) + 255) / 256 * 256;
    int rc = eval_scratch(h, sb + (logits_out ? 0 : (size_t)N * sizeof(float)), s);
    if (rc) return rc;
    float* logits = logits_out ? logits_out : (float*)((char*)h->eval_ws + sb);
    std::string err;
    if (lg_cnn_take_error(&h->cnn)) return fail(h, LG_ERR_HIP, "lg_cnn_evaluate: a split item of the previous forward did not receive its parts");
    {
        ProfScope ps(h, "cnn", s);
        rc = lg_cnn_run(&h->cnn, patches, false, N, logits, s, &err);
    }
    if (rc) return fail(h, rc, err.c_str());
    LG_HIP(h, hipGetLastError());
    rc = eval_run(h, logits, labels, N, chunk, pos_weight, threshold, out, s);
    if (rc) return rc;
    if (lg_cnn_take_error(&h->cnn)) return fail(h, LG_ERR_HIP, "lg_cnn_evaluate: a split CNN item did not receive its parts");
    return LG_OK;
}

static int lg_select_grasp_impl(lg_handle h, const float* depth, const uint8_t* mask, const int16_t* labels, int B, int H, int W,
                                const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                                lg_grasp_result* results, lg_grasp_candidate* cands, void* stream_);
static int lg_select_grasp_labels_impl(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B,
                                       int H, int W, const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                                       lg_grasp_result* results, lg_grasp_candidate* cands, void* stream_);

int lg_select_grasp(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                    float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, lg_grasp_result* results, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    return lg_select_grasp_impl(h, depth, mask, nullptr, B, H, W, pin, out_maps, out_valid, results, nullptr, stream_);
}

// lg_select_grasp on mask[b] = (labels[b] == leaf_ids[b]): the node's `optimal_mask = mask_tensor == optimal_leaf_id` followed by
// select_grasp_point (leaf_grasp_node_v3.py:118-125), the comparison folded into the bit-row pass.
int lg_select_grasp_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W,
                           const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, lg_grasp_result* results,
                           void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    return lg_select_grasp_labels_impl(h, depth, labels, leaf_ids, B, H, W, pin, out_maps, out_valid, results, nullptr, stream_);
}

// Every candidate ranked (lg_candidates_kernel after lg_finish_kernel): the sparse-plane path, no plane outputs
int lg_select_grasp_candidates(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                               lg_grasp_result* results, lg_grasp_candidate* cands, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!cands) return fail(h, LG_ERR_INVALID, "lg_select_grasp_candidates: cands is null");
    return lg_select_grasp_impl(h, depth, mask, nullptr, B, H, W, pin, nullptr, nullptr, results, cands, stream_);
}

int lg_select_grasp_candidates_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B,
                                      int H, int W, const lg_params* pin, lg_grasp_result* results, lg_grasp_candidate* cands,
                                      void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!cands) return fail(h, LG_ERR_INVALID, "lg_select_grasp_candidates_labels: cands is null");
    return lg_select_grasp_labels_impl(h, depth, labels, leaf_ids, B, H, W, pin, nullptr, nullptr, results, cands, stream_);
}

int lg_ml_combined_score(double logit, double trad, double* ml, double* confidence, double* combined) {
    if (!ml || !confidence || !combined) return LG_ERR_INVALID;
    lg_ml_combine(logit, trad, ml, confidence, combined);
    return LG_OK;
}

int lg_cnn_candidate_cannot_win(double trad_i, double trad_0) { return lg_cnn_cannot_win(trad_i, trad_0) ? 1 : 0; }

int lg_rank_grasp_candidates(const double* trad, const double* comb, const int32_t* scored, int n, int rescoring, int32_t* order,
                             double* pick, int32_t* by_ml) {
    if (n < 0 || n > 64) return LG_ERR_INVALID;
    if (n == 0) return LG_OK;
    if (!trad || !comb || !scored || !order || !pick || !by_ml) return LG_ERR_INVALID;
    lg_rank_candidates(trad, comb, scored, n, rescoring, order, pick, by_ml);
    return LG_OK;
}

// The labels entries' staging: room for the 0 / 1 mask the bit-row pass derives from the labels, the frames' leaf ids on the device
static int labels_stage(lg_handle h, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W, void* stream_) {
    if (!labels || !leaf_ids || B < 1 || H < 1 || W < 1) return fail(h, LG_ERR_INVALID, "lg_select_grasp_labels: null or empty input");
    LG_HIP(h, hipSetDevice(h->device));
    const size_t need = (size_t)B * H * W;
    if (need > h->mask_ws_cap) {
        if (h->mask_ws) { hipDeviceSynchronize(); hipFree(h->mask_ws); h->mask_ws = nullptr; h->mask_ws_cap = 0; }
        if (hipMalloc((void**)&h->mask_ws, need) != hipSuccess) { (void)hipGetLastError(); return fail(h, LG_ERR_NOMEM, "lg_select_grasp_labels: mask workspace"); }
        h->mask_ws_cap = need;
    }
    if (B > h->ids_cap) {
        if (h->ids_dev) { hipDeviceSynchronize(); hipFree(h->ids_dev); h->ids_dev = nullptr; }
        if (h->ids_host) { hipHostFree(h->ids_host); h->ids_host = nullptr; }
        h->ids_cap = 0;
        if (hipMalloc((void**)&h->ids_dev, sizeof(int32_t) * B) != hipSuccess ||
            hipHostMalloc((void**)&h->ids_host, sizeof(int32_t) * B) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, LG_ERR_NOMEM, "lg_select_grasp_labels: id buffers");
        }
        h->ids_cap = B;
    }
    memcpy(h->ids_host, leaf_ids, sizeof(int32_t) * B);   // (the previous call on this handle has been synchronised: one call in flight)
    LG_HIP(h, hipMemcpyAsync(h->ids_dev, h->ids_host, sizeof(int32_t) * B, hipMemcpyHostToDevice, (hipStream_t)stream_));
    return LG_OK;
}

static int lg_select_grasp_labels_impl(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B,
                                       int H, int W, const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                                       lg_grasp_result* results, lg_grasp_candidate* cands, void* stream_) {
    const int rc = labels_stage(h, labels, leaf_ids, B, H, W, stream_);
    if (rc) return rc;
    return lg_select_grasp_impl(h, depth, h->mask_ws, labels, B, H, W, pin, out_maps, out_valid, results, cands, stream_);
}

static int lg_select_grasp_impl(lg_handle h, const float* depth, const uint8_t* mask, const int16_t* labels, int B, int H, int W,
                                const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                                lg_grasp_result* results, lg_grasp_candidate* cands, void* stream_) {
    if (!results) return fail(h, LG_ERR_INVALID, "lg_select_grasp: results is null");
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, out_maps, out_valid, "lg_select_grasp");
    if (rc) return rc;
    pl.labels = labels;
    if (lg_label_aware_check(&pl.P, labels ? 1 : 0))
        return fail(h, LG_ERR_INVALID, "lg_select_grasp: label_aware needs the label image (lg_select_grasp_labels, lg_select_grasp_candidates_labels)");
    pl.label_aware = pl.P.label_aware != 0;
    pl.sparse = !out_valid;
    for (int i = 0; i < LG_NUM_MAPS; i++) pl.sparse = pl.sparse && !pl.maps[i];
    const lg_params& P = pl.P;
    if (P.top_k < 1 || P.top_k > 64) return fail(h, LG_ERR_INVALID, "lg_select_grasp: top_k must be in [1,64]");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    rc = ensure_ws(h, B, H, W, P.top_k);
    if (rc) return rc;
    h->last_iso_B = 0;   // (this call's distance transform overwrites the fields of an earlier label-aware call)
    if (pl.label_aware) {   // workspace of the mode: on the first call that asks for it
        const size_t words = (size_t)B * H * pl.WW;
        if (words > h->iso_words_cap || B > h->iso_B_cap) {
            hipDeviceSynchronize();
            if (h->iso_others) hipFree(h->iso_others);
            if (h->iso_dil) hipFree(h->iso_dil);
            if (h->iso_mf) hipFree(h->iso_mf);
            h->iso_others = h->iso_dil = nullptr; h->iso_mf = nullptr; h->iso_words_cap = 0; h->iso_B_cap = 0;
            if (hipMalloc((void**)&h->iso_others, sizeof(unsigned long long) * words) != hipSuccess ||
                hipMalloc((void**)&h->iso_dil, sizeof(unsigned long long) * 2 * words) != hipSuccess ||
                hipMalloc((void**)&h->iso_mf, sizeof(uint32_t) * LG_ISO_MF * B) != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, LG_ERR_NOMEM, "lg_select_grasp_labels: label-aware workspace");
            }
            h->iso_words_cap = words; h->iso_B_cap = B;
        }
    }
    if (cands && (size_t)B * P.top_k > h->cand_rows_cap) {   // candidate rows: on the first call that asks for them
        if (h->cand_rows_dev) { hipDeviceSynchronize(); hipFree(h->cand_rows_dev); h->cand_rows_dev = nullptr; }
        if (h->cand_rows_host) { hipHostFree(h->cand_rows_host); h->cand_rows_host = nullptr; }
        h->cand_rows_cap = 0;
        const size_t cap = (size_t)B * P.top_k;
        if (hipMalloc((void**)&h->cand_rows_dev, sizeof(lg_grasp_candidate) * cap) != hipSuccess ||
            hipHostMalloc((void**)&h->cand_rows_host, sizeof(lg_grasp_candidate) * cap) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, LG_ERR_NOMEM, "lg_select_grasp_candidates: candidate rows");
        }
        h->cand_rows_cap = cap;
    }
    const bool use_cnn = h->cnn.loaded;
    // The CNN on the candidates that can still win only (the result row needs no other; the candidates entry reports an ML
    // score for every candidate and scores them all).  Either way no item of the CNN is split: a patch's logit then does not
    // depend on how many patches run beside it, and the rows of both entries, pruned or not, are equal bit for bit.
    const bool prune = use_cnn && !cands && h->opt.cnn_prune && lg_cnn_counts_on_device(&h->cnn);
    h->last_scored = use_cnn ? (long long)B * P.top_k : 0;
    h->last_scored_subs = 0;
    h->last_cnn_B = 0;
    pl.defer = pl.sparse && h->opt.defer_planes;
    // all eight planes are needed when the CNN rescoring runs and the planes are not deferred (deferred: flatness, which the
    // gather still reads); otherwise only distance + traditional
    for (int i = 0; i < LG_NUM_MAPS; i++)
        if (!pl.maps[i] && ((use_cnn && (!pl.defer || i == LG_MAP_FLATNESS)) || i == LG_MAP_DISTANCE || i == LG_MAP_TRADITIONAL)) {
            rc = ensure_ws_map(h, i);
            if (rc) return rc;
            pl.maps[i] = h->ws_maps[i];
        }
    if (!pl.valid) pl.valid = h->ws_valid;
    const int K = P.top_k;
    const size_t px = (size_t)H * W;
    const int tiles = pl.tiles_x * pl.tiles_y;

    // ---- sub-batch pipeline.  Stages per sub-batch k of SB frames:
    //   D(k): bit rows, stem bits, distance sweeps          -- latency bound, 2*SB workgroups  -> s_dt[k&1]
    //   F(k): fused score planes                             -- HBM bound                       -> s_main
    //   T(k): greedy spaced top-k                            -- latency bound, SB workgroups    -> s_topk
    //   G(k): patch gather + CNN                             -- MFMA bound                      -> s_main
    // s_main runs F(0) F(1) G(0) F(2) G(1) ... so T(k) hides behind F(k+1) and the D chain behind everything.
    int SB = B;
    // Measured on MI355X (B=128, 1080p): SB=32 is 14.8 ms/step vs 11.5 ms unpiped -- the chain
    // D(0)->F(0)->T(0) must drain before the first CNN launch, and D's latency does not shrink with SB.
    // Kept for experiments (LG_SUBBATCH=n in the environment when the handle is created); the default is one sub-batch.
    if (h->opt.subbatch > 0 && !pl.label_aware) SB = h->opt.subbatch;   // (the label-aware transforms reuse the sweeps' scratch: one sub-batch)
    const int nsub = (B + SB - 1) / SB;
    const bool piped = nsub > 1;
    std::vector<LgFinalArgs> fargs((size_t)nsub);   // the plane launches' arguments, for the deferred gather
    pl.near = pl.sparse && h->opt.final_near > 0 && h->opt.subbatch == 0 && h->opt.no_skip == 0;
    h->last_near_B = 0;
    hipStream_t sD[2] = {piped ? h->s_dt[0] : s, piped ? h->s_dt[1] : s};
    hipStream_t sM = piped ? h->s_main : s, sT = piped ? h->s_topk : s;
    while ((int)h->ev_pool.size() < 6 * nsub) {
        hipEvent_t e;
        LG_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ev_pool.push_back(e);
    }
    auto EV = [&](int k, int which) { return h->ev_pool[6 * k + which]; };  // 0 prep 1 copy 2 dt 3 final 4 topk 5 done
    if (piped) {  // internal streams start after whatever the caller queued on `s`
        LG_HIP(h, hipEventRecord(h->ev_begin, s));
        for (hipStream_t q : {sD[0], sD[1], sM, sT}) LG_HIP(h, hipStreamWaitEvent(q, h->ev_begin, 0));
    }
    const LgIsoFields iso_fields = {h->tmp, h->iso_mf};   // (label-aware mode; one sub-batch: frame 0 of the call)
    auto enq_G = [&](int k) -> int {
        const int off = k * SB, n = std::min(SB, B - off);
        if (piped) LG_HIP(h, hipStreamWaitEvent(sM, EV(k, 4), 0));
        if (use_cnn) {
            const int32_t* list = prune ? h->surv_list + (size_t)off * K : nullptr;
            const int32_t* count = prune ? h->surv_count + k : nullptr;
            if (prune) {
                ProfScope ps(h, "survivors", sM);
                lg_launch_survivors(h->surv_keep + off, n, K, h->surv_list + (size_t)off * K, h->surv_slot + (size_t)off * K,
                                    h->surv_count + k, sM);
            }
            {
                ProfScope ps(h, "gather", sM);
                const float* mp[LG_NUM_MAPS];
                for (int i = 0; i < LG_NUM_MAPS; i++) mp[i] = pl.maps[i] ? pl.maps[i] + off * px : nullptr;
                lg_launch_gather(depth + off * px, mask + off * px, mp, pl.sparse ? h->tile_state + (size_t)off * tiles : nullptr,
                                 P.flat_scale, n, H, W, K, h->cand_xy + (size_t)off * K * 2,
                                 h->cand_n + off, h->patches + (size_t)off * K * lg_cnn_halo_patch_floats(), true, sM, list, count,
                                 pl.defer ? &fargs[k] : nullptr, pl.label_aware ? &iso_fields : nullptr);
            }
            std::string err;
            {
                ProfScope ps(h, "cnn", sM);
                int r2 = lg_cnn_run(&h->cnn, h->patches + (size_t)off * K * lg_cnn_halo_patch_floats(), true, n * K, h->logits + (size_t)off * K, sM, &err,
                                    false, count);
                if (r2) return fail(h, r2, err.c_str());
            }
        }
        return LG_OK;
    };
    const bool trace = h->opt.trace;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    hipEvent_t tev[6] = {nullptr};
    if (trace) {
        for (auto& e : tev) hipEventCreate(&e);
        hipEventRecord(tev[0], s);
    }
    // bit rows of the whole batch first (one short kernel) so the host never waits behind a distance sweep
    rc = enq_prep(h, pl, 0, B, sD[0], h->ev_prep);
    if (rc) return rc;
    if (piped) LG_HIP(h, hipStreamWaitEvent(sD[1], h->ev_prep, 0));
    for (int k = 0; k < nsub; k++) {
        const int off = k * SB, n = std::min(SB, B - off);
        rc = enq_dt(h, pl, off, n, sD[k & 1]);
        if (rc) return rc;
        if (piped) LG_HIP(h, hipEventRecord(EV(k, 2), sD[k & 1]));
    }
    if (pl.label_aware) {
        // others -> two dilations -> two chamfer-3 transforms, behind the distance transform on the caller's stream: the fields
        // take the sweeps' scratch (h->tmp, [B][2][H][W] words), free from here on.  A frame without another leaf is skipped
        // by every kernel.
        {
            ProfScope ps(h, "iso_dilate", s);
            lg_launch_iso_dilate(h->iso_others, h->iso_dil, h->iso_mf, B, H, W, pl.WW, s);
        }
        {
            ProfScope ps(h, "iso_sweeps", s);
            if (lg_launch_iso_sweeps(h->iso_dil, h->tmp, h->iso_mf, B, H, W, pl.WW, (uint32_t)P.chamfer_init_dist0, s))
                return fail(h, LG_ERR_UNSUPPORTED, "label_aware: width");
        }
    }
    if (trace && !piped) hipEventRecord(tev[1], s);   // after the sweeps
    const double t_enq1 = now();
    const double t_copy = now();
    bool upload_fp = true;
    rc = finish_orient(h, pl, 0, B, &upload_fp);   // theta per frame: device results (or host analysis) while the sweeps run
    if (rc) return rc;
    const double t_orient = now();
    for (int k = 0; k < nsub; k++) {
        const int off = k * SB, n = std::min(SB, B - off);
        if (piped) LG_HIP(h, hipStreamWaitEvent(sM, EV(k, 2), 0));
        rc = enq_final(h, pl, off, n, sM, upload_fp, &fargs[k]);
        if (rc) return rc;
        if (pl.label_aware && pl.maps[LG_MAP_ISOLATION]) {   // stored plane (dense calls, LG_DEFER_PLANES=0): the current leaf's pixels
            ProfScope ps(h, "iso_plane", sM);
            lg_launch_iso_plane(iso_fields, h->bits, h->win, pl.maps[LG_MAP_ISOLATION], B, H, W, pl.WW, P.iso_w_close, P.iso_w_wide,
                                fargs[k].iso_ramp_top, fargs[k].iso_ramp_step, sM);
        }
        if (trace && !piped) hipEventRecord(tev[2], s);   // after the fused planes
        if (piped) {
            LG_HIP(h, hipEventRecord(EV(k, 3), sM));
            LG_HIP(h, hipStreamWaitEvent(sT, EV(k, 3), 0));
        }
        {
            ProfScope ps(h, "topk", sT);
            lg_launch_topk(pl.maps[LG_MAP_TRADITIONAL] + off * px, pl.valid + off * px, depth + off * px,
                           h->tilekeys + (size_t)off * tiles, pl.sparse ? h->tile_state + (size_t)off * tiles : nullptr,
                           P.flat_scale, P.w_flat, true, n, H, W, K, P.nms_min_distance,
                           h->cand_xy + (size_t)off * K * 2, h->cand_n + off, h->cand_info + (size_t)off * K * 2, sT,
                           prune ? h->surv_keep + off : nullptr, P.mask_is_bool);
        }
        if (trace && !piped) hipEventRecord(tev[3], s);   // after top-k
        if (piped) LG_HIP(h, hipEventRecord(EV(k, 4), sT));
        if (k >= 1) { rc = enq_G(k - 1); if (rc) return rc; }
    }
    rc = enq_G(nsub - 1);
    if (rc) return rc;
    if (prune) h->last_scored_subs = nsub;
    if (trace && !piped) hipEventRecord(tev[4], s);       // after gather + CNN
    if (piped) {  // join: the caller's stream continues after every internal stream
        for (hipStream_t q : {sD[0], sD[1], sM, sT}) {
            LG_HIP(h, hipEventRecord(EV(0, 5), q));
            LG_HIP(h, hipStreamWaitEvent(s, EV(0, 5), 0));
            LG_HIP(h, hipStreamSynchronize(q));
        }
    }
    // ---- the rest of select_grasp_point per frame -- rescoring, 3-D point, pre-grasp probes -- on the device (lg_finish_kernel);
    //      one copy of B result rows comes back
    {
        LgFinishArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.cand_n = h->cand_n; fa.cand_xy = h->cand_xy; fa.cand_info = h->cand_info; fa.logits = h->logits;
        fa.slot = prune ? h->surv_slot : nullptr; fa.slot_frames = SB;
        fa.bits2 = pl.label_aware ? h->iso_others : nullptr;
        fa.fp = h->fp_dev; fa.bits = h->bits; fa.out = h->res_host_dev ? h->res_host_dev : h->res_dev;
        fa.B = B; fa.H = H; fa.W = W; fa.WW = pl.WW; fa.K = K; fa.use_cnn = use_cnn ? 1 : 0; fa.mask_is_bool = P.mask_is_bool;
        fa.cx = P.cx; fa.cy = P.cy; fa.f = P.f;
        lg_make_se_spans(2 * P.pregrasp_clearance + 1, &fa.se);
        {
            ProfScope ps(h, "finish", s);
            lg_launch_finish(fa, s);
        }
        if (cands) {
            ProfScope ps(h, "candidates", s);
            lg_launch_candidates(fa, h->cand_rows_dev, s);
        }
    }
    // (with a device alias lg_finish_kernel wrote the rows into res_host itself: they are there behind the synchronise below)
    if (!h->res_host_dev)
        LG_HIP(h, hipMemcpyAsync(h->res_host, h->res_dev, sizeof(lg_grasp_result) * B, hipMemcpyDeviceToHost, s));
    if (cands)
        LG_HIP(h, hipMemcpyAsync(h->cand_rows_host, h->cand_rows_dev, sizeof(lg_grasp_candidate) * B * K, hipMemcpyDeviceToHost, s));
    const double t_enq2 = now();
    LG_HIP(h, hipStreamSynchronize(s));
    const double t_sync = now();
    LG_HIP(h, hipGetLastError());
    if (use_cnn && lg_cnn_take_error(&h->cnn)) return fail(h, LG_ERR_HIP, "lg_select_grasp: a split CNN item did not receive its parts");
    memcpy(results, h->res_host, sizeof(lg_grasp_result) * B);
    if (cands) memcpy(cands, h->cand_rows_host, sizeof(lg_grasp_candidate) * B * K);
    if (use_cnn) { h->last_cnn_B = B; h->last_cnn_K = K; h->last_cnn_SB = SB; h->last_cnn_pruned = prune; }
    h->last_patch_floats = use_cnn ? (long long)B * K * lg_cnn_halo_patch_floats() : 0;
    if (pl.near) h->last_near_B = B;
    if (pl.label_aware) { h->last_iso_B = B; h->last_iso_H = H; h->last_iso_W = W; }
    if (trace && !piped) {
        float a[5] = {0};
        for (int i = 1; i <= 4; i++) hipEventElapsedTime(&a[i], tev[0], tev[i]);
        fprintf(stderr, "[lg] gpu timeline (ms since call start): sweeps done %.3f | planes %.3f | topk %.3f | cnn %.3f\n", a[1], a[2],
                a[3], a[4]);
    }
    if (trace) for (auto& e : tev) if (e) hipEventDestroy(e);
    if (trace)
        fprintf(stderr, "[lg] B=%d enq1 %.3f | wait bits %.3f | orient %.3f | enq2 %.3f | gpu wait %.3f | post %.3f ms\n", B,
                t_enq1 - t_start, t_copy - t_enq1, t_orient - t_copy, t_enq2 - t_orient, t_sync - t_enq2, now() - t_sync);
    return LG_OK;
}

// ============================================================================ ML-only grasp selection (lg_mlsel.h)
void lg_default_ml_sampling(lg_ml_sampling* s) {
    if (!s) return;
    s->mode = LG_ML_SAMPLE_NTH; s->target = 100; s->stride = 8; s->max_samples = 4096; s->chunk = 0;
}

// The table of one frame on the host: row counts and their prefix over every row, then lg_ml_locate per sample -- the functions
// lg_ml_rows_kernel and lg_ml_table_kernel call (the device walks the bounding-box rows only; the other rows count nothing).
int lg_ml_sample_points_host(const uint64_t* bits_, int H, int W, int WW, const lg_ml_sampling* sp, int32_t* xy, int32_t* scored,
                             int cap, int32_t* n, int64_t sums[3]) {
    if (!bits_ || !n || H < 1 || W < 1 || WW != (W + 63) / 64 || cap < 1 || lg_ml_sampling_error(sp)) return LG_ERR_INVALID;
    lg_ml_sampling s = *sp;
    if (cap < s.max_samples) s.max_samples = cap;
    if (lg_ml_sampling_error(&s)) return LG_ERR_INVALID;   // (NTH: the 2 target - 1 samples must fit)
    const unsigned long long* bits = (const unsigned long long*)bits_;
    LgMlFrame f;
    memset(&f, 0, sizeof(f));
    f.y0 = 0; f.rows = H; f.w0 = 0; f.w1 = WW - 1;
    std::vector<int32_t> pre((size_t)H);
    int run = 0;
    for (int y = 0; y < H; y++) {
        pre[y] = run;
        const bool on = lg_ml_row_sampled(s.mode, s.stride, y);
        for (int w = 0; w < WW; w++) {
            const unsigned long long v = bits[(size_t)y * WW + w];
            const int c = lg_ml_popc(v);
            f.area += c;
            f.sx += (long long)c * (64 * w) + lg_ml_index_sum(v);
            f.sy += (long long)c * y;
            if (on) run += lg_ml_popc(v & lg_ml_pattern(s.mode, s.stride, w));
        }
    }
    f.total = run;
    lg_ml_frame_counts(s, &f);
    *n = f.n;
    if (sums) { sums[0] = f.sx; sums[1] = f.sy; sums[2] = f.area; }
    for (int i = 0; i < f.n; i++) {
        int x, y, sc;
        lg_ml_locate(bits, H, W, WW, s, f, pre.data(), i, &x, &y, &sc);
        if (xy) { xy[2 * i] = x; xy[2 * i + 1] = y; }
        if (scored) scored[i] = sc;
    }
    return LG_OK;
}

int lg_debug_ml_planes(lg_handle h, int form, int32_t* last) {
    if (!h || form < 0 || form > 2) return LG_ERR_INVALID;
    LG_ENTER(h);
    h->ml_planes = form;
    if (last) *last = h->ml_last_form;
    return LG_OK;
}

static int ml_ensure(lg_ctx* h, int B, int H, int M, int chunk, bool want_rows) {
    const size_t BM = (size_t)B * M, BH = (size_t)B * H;
    if (BM > h->ml_cap_BM || BH > h->ml_cap_BH || B > h->ml_cap_B) {
        hipDeviceSynchronize();
        const size_t nBM = std::max(BM, h->ml_cap_BM), nBH = std::max(BH, h->ml_cap_BH);
        const int nB = std::max(B, h->ml_cap_B);
        {
            auto F = [](void* p) { if (p) hipFree(p); };
            LgMlBuffers& m = h->ml;
            F(m.frames); F(m.row_pre); F(m.xy); F(m.scored); F(m.slot_local); F(m.list); F(m.slot); F(m.counts); F(m.n_frame); F(m.logits);
            F(m.pick_n); F(m.pick_xy); F(m.pick_info); F(m.pick_meta);
            m = LgMlBuffers{};
            if (h->ml_counts_host) hipHostFree(h->ml_counts_host);
            h->ml_counts_host = nullptr;
            h->ml_cap_BM = h->ml_cap_BH = 0; h->ml_cap_B = 0;
        }
        LgMlBuffers& m = h->ml;
        LG_HIP(h, dev_alloc(&m.frames, (size_t)nB));
        LG_HIP(h, dev_alloc(&m.row_pre, nBH));
        LG_HIP(h, dev_alloc(&m.xy, nBM * 2));
        LG_HIP(h, dev_alloc(&m.scored, nBM));
        LG_HIP(h, dev_alloc(&m.slot_local, nBM));
        LG_HIP(h, dev_alloc(&m.list, nBM));
        LG_HIP(h, dev_alloc(&m.slot, nBM));
        LG_HIP(h, dev_alloc(&m.counts, (size_t)nB * 2));
        LG_HIP(h, dev_alloc(&m.n_frame, (size_t)nB));
        LG_HIP(h, dev_alloc(&m.logits, nBM));
        LG_HIP(h, dev_alloc(&m.pick_n, (size_t)nB));
        LG_HIP(h, dev_alloc(&m.pick_xy, (size_t)nB * 2));
        LG_HIP(h, dev_alloc(&m.pick_info, (size_t)nB * 2));
        LG_HIP(h, dev_alloc(&m.pick_meta, (size_t)nB * 4));
        LG_HIP(h, hipHostMalloc((void**)&h->ml_counts_host, sizeof(int32_t) * 2 * nB));
        h->ml_cap_BM = nBM; h->ml_cap_BH = nBH; h->ml_cap_B = nB;
    }
    const size_t n_chunks = (BM + chunk - 1) / chunk;
    if (n_chunks > h->ml_chunk_cap) {
        hipDeviceSynchronize();
        if (h->ml_chunk_dev) hipFree(h->ml_chunk_dev);
        if (h->ml_chunk_host) hipHostFree(h->ml_chunk_host);
        h->ml_chunk_dev = nullptr; h->ml_chunk_host = nullptr; h->ml_chunk_cap = 0;
        LG_HIP(h, dev_alloc(&h->ml_chunk_dev, n_chunks));
        LG_HIP(h, hipHostMalloc((void**)&h->ml_chunk_host, sizeof(int32_t) * n_chunks));
        h->ml_chunk_cap = n_chunks;
    }
    if (chunk > h->ml_patches_cap) {
        hipDeviceSynchronize();
        if (h->ml_patches) hipFree(h->ml_patches);
        h->ml_patches = nullptr; h->ml_patches_cap = 0;
        const size_t fl = (size_t)chunk * lg_cnn_halo_patch_floats();
        LG_HIP(h, dev_alloc(&h->ml_patches, fl));
        LG_HIP(h, hipMemset(h->ml_patches, 0, fl * sizeof(float)));   // the halos and the three spare planes stay zero
        h->ml_patches_cap = chunk;
    }
    if (want_rows && BM > h->ml_rows_cap) {
        hipDeviceSynchronize();
        if (h->ml_rows) hipFree(h->ml_rows);
        h->ml_rows = nullptr; h->ml_rows_cap = 0;
        LG_HIP(h, dev_alloc(&h->ml_rows, BM));
        h->ml_rows_cap = BM;
    }
    if (!h->ev_ml) LG_HIP(h, hipEventCreateWithFlags(&h->ev_ml, hipEventDisableTiming));
    return LG_OK;
}

// lg_select_grasp_impl's front (bit rows, distance transform, orientation, the sparse near-tile plane launch) without top-k;
// then the sample table's scored windows through the gather and the CNN in chunks, the pick, lg_finish_kernel on the one-point list.
static int lg_select_grasp_ml_impl(lg_handle h, const float* depth, const uint8_t* mask, const int16_t* labels, int B, int H, int W,
                                   const lg_params* pin, const lg_ml_sampling* sp, lg_grasp_result* results, lg_ml_sample* samples,
                                   int32_t* n_samples, void* stream_) {
    if (!results) return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: results is null");
    lg_ml_sampling S;
    if (sp) S = *sp; else lg_default_ml_sampling(&S);
    if (const char* why = lg_ml_sampling_error(&S)) return fail(h, LG_ERR_INVALID, (std::string("lg_select_grasp_ml: ") + why).c_str());
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, nullptr, nullptr, "lg_select_grasp_ml");
    if (rc) return rc;
    pl.labels = labels;
    if (lg_label_aware_check(&pl.P, labels ? 1 : 0))
        return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: label_aware needs the label image (lg_select_grasp_ml_labels)");
    if ((size_t)B * S.max_samples > 0x7fffffffull) return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: B * max_samples must stay below 2^31");
    pl.label_aware = pl.P.label_aware != 0;
    pl.sparse = true;
    const lg_params& P = pl.P;
    const int M = S.max_samples, chunk = S.chunk > 0 ? S.chunk : LG_ML_DEFAULT_CHUNK;
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    rc = ensure_ws(h, B, H, W, std::max(P.top_k, 1));
    if (rc) return rc;
    rc = ml_ensure(h, B, H, M, chunk, samples != nullptr);
    if (rc) return rc;
    h->last_iso_B = 0;
    if (pl.label_aware) {   // workspace of the mode, as lg_select_grasp_impl
        const size_t words = (size_t)B * H * pl.WW;
        if (words > h->iso_words_cap || B > h->iso_B_cap) {
            hipDeviceSynchronize();
            if (h->iso_others) hipFree(h->iso_others);
            if (h->iso_dil) hipFree(h->iso_dil);
            if (h->iso_mf) hipFree(h->iso_mf);
            h->iso_others = h->iso_dil = nullptr; h->iso_mf = nullptr; h->iso_words_cap = 0; h->iso_B_cap = 0;
            if (hipMalloc((void**)&h->iso_others, sizeof(unsigned long long) * words) != hipSuccess ||
                hipMalloc((void**)&h->iso_dil, sizeof(unsigned long long) * 2 * words) != hipSuccess ||
                hipMalloc((void**)&h->iso_mf, sizeof(uint32_t) * LG_ISO_MF * B) != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, LG_ERR_NOMEM, "lg_select_grasp_ml_labels: label-aware workspace");
            }
            h->iso_words_cap = words; h->iso_B_cap = B;
        }
    }
    const bool use_cnn = h->cnn.loaded;
    // Where the gather finds sdf, approach, isolation, accessibility and stem: computed at every window's pixels (deferred), or
    // stored once by the plane kernel on the leaf's tiles.  Overlapping GRID windows recompute a pixel up to (32 / stride)^2
    // times in the deferred form, yet at 1080p the gather takes the same time either way (GRID / 8, 32 frames, 46296 windows:
    // 1.265 against 1.269 ms; NTH / 100: 0.108 against 0.111) and the score-only plane kernel is the cheaper one (0.034 against
    // 0.046 ms): deferred always, which also keeps five planes out of the workspace (profiles/NOTES_ml_select.md).
    const int form = h->ml_planes ? h->ml_planes : h->opt.defer_planes ? 1 : 2;
    pl.defer = form == 1;
    h->ml_last_form = form;
    h->last_scored = 0; h->last_scored_subs = 0; h->last_cnn_B = 0; h->last_patch_floats = 0; h->last_near_B = 0;
    for (int i = 0; i < LG_NUM_MAPS; i++)
        if ((use_cnn && (!pl.defer || i == LG_MAP_FLATNESS)) || i == LG_MAP_DISTANCE || i == LG_MAP_TRADITIONAL) {
            rc = ensure_ws_map(h, i);
            if (rc) return rc;
            pl.maps[i] = h->ws_maps[i];
        }
    pl.valid = h->ws_valid;
    pl.near = h->opt.final_near > 0 && h->opt.subbatch == 0 && h->opt.no_skip == 0;
    const size_t px = (size_t)H * W;
    (void)px;
    const LgMlBuffers& m = h->ml;
    rc = enq_prep(h, pl, 0, B, s, h->ev_prep);
    if (rc) return rc;
    // the table needs the bit rows and the bounding boxes only: it runs in front of the distance transform and the host reads
    // its counts behind ev_ml, after everything up to the plane kernel has been queued
    {
        ProfScope ps(h, "ml_rows", s);
        lg_launch_ml_rows(h->bits, h->win, S, m, B, H, W, pl.WW, s);
    }
    {
        ProfScope ps(h, "ml_table", s);
        lg_launch_ml_table(h->bits, S, m, B, H, W, pl.WW, s);
    }
    {
        ProfScope ps(h, "ml_list", s);
        lg_launch_ml_list(S, m, B, s);
    }
    LG_HIP(h, hipMemcpyAsync(h->ml_counts_host, m.counts, sizeof(int32_t) * 2 * B, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipEventRecord(h->ev_ml, s));
    rc = enq_dt(h, pl, 0, B, s);
    if (rc) return rc;
    const LgIsoFields iso_fields = {h->tmp, h->iso_mf};
    if (pl.label_aware) {
        {
            ProfScope ps(h, "iso_dilate", s);
            lg_launch_iso_dilate(h->iso_others, h->iso_dil, h->iso_mf, B, H, W, pl.WW, s);
        }
        {
            ProfScope ps(h, "iso_sweeps", s);
            if (lg_launch_iso_sweeps(h->iso_dil, h->tmp, h->iso_mf, B, H, W, pl.WW, (uint32_t)P.chamfer_init_dist0, s))
                return fail(h, LG_ERR_UNSUPPORTED, "label_aware: width");
        }
    }
    bool upload_fp = true;
    rc = finish_orient(h, pl, 0, B, &upload_fp);
    if (rc) return rc;
    LgFinalArgs fargs;
    rc = enq_final(h, pl, 0, B, s, upload_fp, &fargs);
    if (rc) return rc;
    if (pl.label_aware && pl.maps[LG_MAP_ISOLATION]) {   // stored planes: the current leaf's pixels
        ProfScope ps(h, "iso_plane", s);
        lg_launch_iso_plane(iso_fields, h->bits, h->win, pl.maps[LG_MAP_ISOLATION], B, H, W, pl.WW, P.iso_w_close, P.iso_w_wide,
                            fargs.iso_ramp_top, fargs.iso_ramp_step, s);
    }
    LG_HIP(h, hipEventSynchronize(h->ev_ml));   // (the table kernels ended long ago: they follow the bit-row pass)
    long long total = 0;
    for (int b = 0; b < B; b++) total += h->ml_counts_host[2 * b + 1];
    if (use_cnn && total > 0) {
        const int n_chunks = (int)((total + chunk - 1) / chunk);
        for (int c = 0; c < n_chunks; c++) h->ml_chunk_host[c] = (int32_t)std::min<long long>(chunk, total - (long long)c * chunk);
        LG_HIP(h, hipMemcpyAsync(h->ml_chunk_dev, h->ml_chunk_host, sizeof(int32_t) * n_chunks, hipMemcpyHostToDevice, s));
        const float* mp[LG_NUM_MAPS];
        for (int i = 0; i < LG_NUM_MAPS; i++) mp[i] = pl.maps[i];
        for (int c = 0; c < n_chunks; c++) {
            const int nc = h->ml_chunk_host[c];
            {
                // patch slot j of the pass takes list entry c * chunk + j = frame * M + sample; the grid covers nc slots
                ProfScope ps(h, "gather", s);
                lg_launch_gather(depth, mask, mp, h->tile_state, P.flat_scale, (nc + M - 1) / M, H, W, M, m.xy, m.n_frame, h->ml_patches,
                                 true, s, m.list + (size_t)c * chunk, h->ml_chunk_dev + c, pl.defer ? &fargs : nullptr,
                                 pl.label_aware && pl.defer ? &iso_fields : nullptr);
            }
            std::string err;
            {
                // no item split (a logit does not depend on what runs beside it), exactly nc patches
                ProfScope ps(h, "cnn", s);
                const int r2 = lg_cnn_run(&h->cnn, h->ml_patches, true, nc, m.logits + (size_t)c * chunk, s, &err, false, nullptr);
                if (r2) return fail(h, r2, err.c_str());
            }
        }
        h->last_scored = total;
    }
    {
        ProfScope ps(h, "ml_pick", s);
        lg_launch_ml_pick(depth, m, M, B, H, W, use_cnn ? 1 : 0, s);
    }
    lg_grasp_result* const res_out = h->res_host_dev ? h->res_host_dev : h->res_dev;
    {
        LgFinishArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.cand_n = m.pick_n; fa.cand_xy = m.pick_xy; fa.cand_info = m.pick_info; fa.logits = nullptr; fa.slot = nullptr; fa.slot_frames = B;
        fa.bits2 = pl.label_aware ? h->iso_others : nullptr;
        fa.fp = h->fp_dev; fa.bits = h->bits; fa.out = res_out;
        fa.B = B; fa.H = H; fa.W = W; fa.WW = pl.WW; fa.K = 1; fa.use_cnn = 0; fa.mask_is_bool = P.mask_is_bool;
        fa.cx = P.cx; fa.cy = P.cy; fa.f = P.f;
        lg_make_se_spans(2 * P.pregrasp_clearance + 1, &fa.se);
        ProfScope ps(h, "finish", s);
        lg_launch_finish(fa, s);
    }
    {
        ProfScope ps(h, "ml_rows_out", s);
        lg_launch_ml_rows_out(m, M, B, use_cnn ? 1 : 0, res_out, samples ? h->ml_rows : nullptr, s);
    }
    if (!h->res_host_dev)
        LG_HIP(h, hipMemcpyAsync(h->res_host, h->res_dev, sizeof(lg_grasp_result) * B, hipMemcpyDeviceToHost, s));
    if (samples) LG_HIP(h, hipMemcpyAsync(samples, h->ml_rows, sizeof(lg_ml_sample) * (size_t)B * M, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    LG_HIP(h, hipGetLastError());
    if (use_cnn && lg_cnn_take_error(&h->cnn)) return fail(h, LG_ERR_HIP, "lg_select_grasp_ml: a split CNN item did not receive its parts");
    memcpy(results, h->res_host, sizeof(lg_grasp_result) * B);
    if (n_samples)
        for (int b = 0; b < B; b++) n_samples[b] = h->ml_counts_host[2 * b];
    if (pl.near) h->last_near_B = B;
    if (pl.label_aware) { h->last_iso_B = B; h->last_iso_H = H; h->last_iso_W = W; }
    return LG_OK;
}

int lg_select_grasp_ml(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                       const lg_ml_sampling* sampling, lg_grasp_result* results, lg_ml_sample* samples, int32_t* n_samples, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    return lg_select_grasp_ml_impl(h, depth, mask, nullptr, B, H, W, pin, sampling, results, samples, n_samples, stream_);
}

int lg_select_grasp_ml_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W,
                              const lg_params* pin, const lg_ml_sampling* sampling, lg_grasp_result* results, lg_ml_sample* samples,
                              int32_t* n_samples, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    const int rc = labels_stage(h, labels, leaf_ids, B, H, W, stream_);
    if (rc) return rc;
    return lg_select_grasp_ml_impl(h, depth, h->mask_ws, labels, B, H, W, pin, sampling, results, samples, n_samples, stream_);
}

}  // extern "C"
