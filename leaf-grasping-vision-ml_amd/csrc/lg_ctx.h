// The handle behind lg_handle and what every host translation unit of it needs (lg_api.hip: create / destroy, errors, profiling,
// the debug and single-stage entries; lg_select.hip: the workspaces and the grasp-selection entries).  Private to csrc/.
#pragma once
#include <math.h>
#include <stdio.h>

#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "lg_cnn.h"
#include "lg_collect.h"
#include "lg_internal.h"
#include "lg_leaf.h"
#include "lg_midrib.h"
#include "lg_mlsel.h"
#include "lg_options.h"
#include "lg_orient.h"
#include "lg_pool.h"

struct LgProfSlot {
    std::string name;
    std::vector<hipEvent_t> ev;  // pairs
    std::vector<uint8_t> cont;   // per pair: it continues a launch of this call that another pair counts (ProfScope, lg_ctx::prof_cont)
    size_t used = 0;
    int launches = 0;
    double total_ms = 0.0;
};

struct lg_ctx {
    int device = 0;
    std::string err;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_prep = nullptr, ev_copy = nullptr;
    // library streams of lg_select_grasp*: the stages of the LG_SUBBATCH pipeline (schedule_subbatches) and lanes 1 .. of the
    // tail in lanes (schedule_lanes, LG_TAIL_LANE_STREAMS); s_dt also takes the row search and the small batches' side tail
    hipStream_t s_dt[2] = {nullptr, nullptr}, s_main = nullptr, s_topk = nullptr;
    std::vector<hipEvent_t> ev_pool;  // untimed events of both, four per frame range (lg_select.hip: EV_DT .. EV_DONE)
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
    // true while the call queues lanes 1 .. of its tail (schedule_lanes): a scope opened now continues the launch that lane
    // 0 counted -- prof_flush adds its milliseconds to the slot without counting a launch, so a slot reads one launch per call
    // and the sum of its lanes' times (which overlap: the slots of a call in lanes add up to more than its wall time)
    bool prof_cont = false;
    // tail lanes of lg_select_grasp* (lg_debug_tail_lanes): the request -- 0: the automatic rule, 1 .. 4: that many lanes wherever
    // lanes are allowed -- and the lanes of the last call
    int tail_lanes_req = 0, last_tail_lanes = 0;
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
    LgColWs col;                          // lg_select_grasp_collect, lg_erode_ellipse, lg_argmax_first (lg_collect.h), grown on demand
};

namespace {   // (every translation unit takes its own copy, as when all of this lived in one file: nothing here is exported)

inline int fail(lg_handle h, int code, const char* what, hipError_t e = hipSuccess) {
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
            slot->cont.push_back(0);
        }
        slot->cont[slot->used / 2] = h->prof_cont ? 1 : 0;
        e0 = slot->ev[slot->used];
        if (!ext) hipEventRecord(e0, s);
        e1 = slot->ev[slot->used + 1];
        slot->used += 2;
    }
    ~ProfScope() {
        if (slot && e1 && !ext) hipEventRecord(e1, s);
    }
};

inline void prof_flush(lg_ctx* h) {  // resolve recorded pairs into totals (call after a synchronise)
    for (auto& p : h->prof) {
        for (size_t i = 0; i + 1 < p.used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) == hipSuccess) {
                p.total_ms += ms;
                if (!p.cont[i / 2]) p.launches++;
            }
        }
        p.used = 0;
    }
}

template <typename T>
inline hipError_t dev_alloc(T** p, size_t n) {
    return hipMalloc((void**)p, n * sizeof(T));
}

inline void parallel_for(lg_ctx* h, int n, const std::function<void(int)>& fn) {
    if (h->pool && n > 1) h->pool->run(n, fn);
    else
        for (int i = 0; i < n; i++) fn(i);
}

// ImageProcessor._create_gaussian_kernel (image_processor.py:25-32): the 2-D kernel exp(-(dx^2 + dy^2) / 2 sigma^2) / sum with
// sigma = size / 6 is the outer product of this 1-D factor with itself
inline void gaussian1d(int size, float* k1) {
    const double sigma = size / 6.0;
    const int c = size / 2;
    double e[LG_MAX_GAUSS], s = 0;
    for (int i = 0; i < size; i++) { e[i] = exp(-((i - c) * (i - c)) / (2 * sigma * sigma)); s += e[i]; }
    for (int i = 0; i < size; i++) k1[i] = (float)(e[i] / s);
}

}  // namespace

// lg_select.hip, for the entries of lg_api.hip that borrow the selection workspace and for lg_destroy (not exported)
#define LG_LOCAL __attribute__((visibility("hidden")))
LG_LOCAL int ensure_ws(lg_ctx* h, int B, int H, int W, int K);
LG_LOCAL void free_ws(lg_ctx* h);
LG_LOCAL void ml_free(lg_ctx* h);
LG_LOCAL void col_free(lg_ctx* h);
