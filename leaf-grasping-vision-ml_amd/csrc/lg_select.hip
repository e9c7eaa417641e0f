// Grasp selection behind the C-ABI (include/leafgrasp.h): the handle's workspaces, the stages every entry queues (bit rows, distance
// transform, label-aware fields, orientation, plane kernel, lg_finish_kernel, result rows) and the entries themselves --
// lg_score_maps, lg_select_grasp* (top-k candidates, CNN rescoring) and lg_select_grasp_ml* (CNN over sampled leaf pixels).
// Host orchestration only; no exceptions cross the boundary.
#include <string.h>

#include <algorithm>
#include <chrono>

#include "lg_ctx.h"
#include "lg_dt.h"

// Tail lanes of lg_select_grasp* (lg_tail_lane_plan): the automatic rule -- LG_TAIL_LANES_AUTO lanes from LG_TAIL_LANES_MIN_B
// frames on, one lane below -- and the library streams of lanes 1, 2, 3 (members of the handle `h`).
// profiles/NOTES_tail_lanes.md has the readings behind all three (tools/tail_lanes_ab.py, 1080p, ms per step, three rounds):
//   256 frames: 1 lane 1.886 .. 1.897, 2 lanes 1.816 .. 1.820, 3 lanes 2.225 .. 2.238, 4 lanes 2.249 .. 2.267
//   128 frames: 1.162 .. 1.165 / 1.254 .. 1.256 / 1.572 .. 1.573 / 1.616 .. 1.623;  64: 0.937 .. 0.947 / 0.993 .. 1.004;  32: 0.742 .. 0.743 / 0.749 .. 0.753
// Two lanes win every round at 256 frames and lose at 128 and below; three and four lose everywhere.  Lane 1 on s_dt[0]
// instead of s_main: 1.808 .. 1.813 against 1.881 .. 1.884 ms, the same gain -- neither lands on the caller's hardware queue.
#ifndef LG_TAIL_LANES_AUTO
#define LG_TAIL_LANES_AUTO 2
#endif
#ifndef LG_TAIL_LANES_MIN_B
#define LG_TAIL_LANES_MIN_B 256
#endif
#ifndef LG_TAIL_LANE_STREAMS
#define LG_TAIL_LANE_STREAMS h->s_main, h->s_topk, h->s_dt[0]
#endif

// ============================================================================ workspaces
namespace {

std::atomic<int> g_select_in_flight{0};   // lg_select_grasp* calls of this process that are running now, on any handle (tail lanes)

// the inspection fields a selection call owns (lg_debug_near_tiles, _isolation_fields, _cnn_scored, _cnn_survivors, _patch):
// cleared when the call starts and when the workspace goes, set again by what the call does
void reset_last(lg_ctx* h) {
    h->last_near_B = 0; h->last_iso_B = 0;
    h->last_tail_lanes = 0;
    h->last_scored = 0; h->last_scored_subs = 0; h->last_cnn_B = 0; h->last_patch_floats = 0;
}

template <typename T>
void free_dev(T*& p) { if (p) hipFree(p); p = nullptr; }
template <typename T>
void free_pinned(T*& p) { if (p) hipHostFree(p); p = nullptr; }

// A buffer grown on demand: what it held is released (behind a device synchronise: a kernel may still read it) and n elements
// are allocated.  The caller tests and sets the capacity -- several buffers may share one -- and words the failure.
template <typename T>
hipError_t regrow_dev(T** p, size_t n) {
    if (*p) hipDeviceSynchronize();
    free_dev(*p);
    const hipError_t e = dev_alloc(p, n);
    if (e != hipSuccess) (void)hipGetLastError();   // (sticky until read: it must not fail the next call)
    return e;
}
template <typename T>
hipError_t regrow_pinned(T** p, size_t n) {
    free_pinned(*p);
    const hipError_t e = hipHostMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

}  // namespace

void free_ws(lg_ctx* h) {
    free_dev(h->tmp); free_dev(h->bits); free_dev(h->stem); free_dev(h->tilekeys); free_dev(h->tile_state); free_dev(h->maxfix);
    free_dev(h->win); free_dev(h->fp_dev); free_dev(h->near_off); free_dev(h->res_dev);
    for (float*& m : h->ws_maps) free_dev(m);
    free_dev(h->ws_valid); free_dev(h->cand_xy); free_dev(h->cand_n); free_dev(h->cand_info); free_dev(h->patches); free_dev(h->logits);
    free_dev(h->surv_keep); free_dev(h->surv_list); free_dev(h->surv_slot); free_dev(h->surv_count);
    free_pinned(h->fp_host); free_pinned(h->bits_host); free_pinned(h->win_host); free_pinned(h->res_host); free_pinned(h->near_off_host);
    h->bits_host_dev = nullptr; h->near_off_host_dev = nullptr; h->fp_host_dev = nullptr; h->res_host_dev = nullptr;
    reset_last(h);
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

namespace {

int ensure_ws_map(lg_ctx* h, int i) {  // internal plane when the caller does not want map i
    if (h->ws_maps[i]) return LG_OK;
    LG_HIP(h, dev_alloc(&h->ws_maps[i], (size_t)h->capB * h->capH * h->capW));
    return LG_OK;
}

void ml_free_table(lg_ctx* h) {   // the sample table and what follows it, with the pinned counts (one capacity triple)
    LgMlBuffers& m = h->ml;
    free_dev(m.frames); free_dev(m.row_pre); free_dev(m.xy); free_dev(m.scored); free_dev(m.slot_local); free_dev(m.list);
    free_dev(m.slot); free_dev(m.counts); free_dev(m.n_frame); free_dev(m.logits);
    free_dev(m.pick_n); free_dev(m.pick_xy); free_dev(m.pick_info); free_dev(m.pick_meta);
    free_pinned(h->ml_counts_host);
    h->ml_cap_BM = h->ml_cap_BH = 0; h->ml_cap_B = 0;
}

}  // namespace

void ml_free(lg_ctx* h) {
    ml_free_table(h);
    free_dev(h->ml_patches); free_dev(h->ml_rows); free_dev(h->ml_chunk_dev); free_pinned(h->ml_chunk_host);
    h->ml_patches_cap = 0; h->ml_rows_cap = 0; h->ml_chunk_cap = 0;
}

void col_free(lg_ctx* h) {   // the collecting entries' workspace (lg_collect.h)
    LgColWs& c = h->col;
    free_dev(c.comp[0]); free_dev(c.comp[1]); free_dev(c.safe);
    for (float*& p : c.planes) free_dev(p);
    free_dev(c.sums); free_dev(c.red.key); free_dev(c.red.any);
    free_dev(c.pick.n); free_dev(c.pick.xy); free_dev(c.pick.info); free_dev(c.pick.meta);
    free_pinned(c.key_host); free_pinned(c.any_host);
    c.cap_words = 0; c.cap_px = 0; c.cap_B = 0;
}

namespace {

// Room for B frames of H x W: the buffers are indexed by the call's own shape, so one capacity per kind is enough.  The float
// planes come on first use (col_plane): a caller who takes every plane back needs none.
int col_ensure(lg_ctx* h, int B, int H, int W) {
    LgColWs& c = h->col;
    const size_t words = (size_t)B * H * ((W + 63) / 64), px = (size_t)B * H * W;
    if (words <= c.cap_words && px <= c.cap_px && B <= c.cap_B) return LG_OK;
    const size_t nw = std::max(words, c.cap_words), np = std::max(px, c.cap_px);
    const int nB = std::max(B, c.cap_B);
    hipDeviceSynchronize();
    col_free(h);
    LG_HIP(h, dev_alloc(&c.comp[0], nw));
    LG_HIP(h, dev_alloc(&c.comp[1], nw));
    LG_HIP(h, dev_alloc(&c.safe, np));
    LG_HIP(h, dev_alloc(&c.sums, (size_t)nB * LG_COL_SUMS));
    LG_HIP(h, dev_alloc(&c.red.key, (size_t)nB));
    LG_HIP(h, dev_alloc(&c.red.any, (size_t)nB));
    LG_HIP(h, dev_alloc(&c.pick.n, (size_t)nB));
    LG_HIP(h, dev_alloc(&c.pick.xy, (size_t)nB * 2));
    LG_HIP(h, dev_alloc(&c.pick.info, (size_t)nB * 2));
    LG_HIP(h, dev_alloc(&c.pick.meta, (size_t)nB * 2));
    LG_HIP(h, hipHostMalloc((void**)&c.key_host, sizeof(unsigned long long) * nB));
    LG_HIP(h, hipHostMalloc((void**)&c.any_host, sizeof(int32_t) * nB));
    c.cap_words = nw; c.cap_px = np; c.cap_B = nB;
    return LG_OK;
}

int col_plane(lg_ctx* h, int i, float** out) {
    LgColWs& c = h->col;
    if (!c.planes[i]) LG_HIP(h, dev_alloc(&c.planes[i], c.cap_px));
    *out = c.planes[i];
    return LG_OK;
}

int ml_ensure(lg_ctx* h, int B, int H, int M, int chunk, bool want_rows) {
    const size_t BM = (size_t)B * M, BH = (size_t)B * H;
    if (BM > h->ml_cap_BM || BH > h->ml_cap_BH || B > h->ml_cap_B) {
        const size_t nBM = std::max(BM, h->ml_cap_BM), nBH = std::max(BH, h->ml_cap_BH);
        const int nB = std::max(B, h->ml_cap_B);
        hipDeviceSynchronize();
        ml_free_table(h);
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
        h->ml_chunk_cap = 0;
        LG_HIP(h, regrow_dev(&h->ml_chunk_dev, n_chunks));
        LG_HIP(h, regrow_pinned(&h->ml_chunk_host, n_chunks));
        h->ml_chunk_cap = n_chunks;
    }
    if (chunk > h->ml_patches_cap) {
        h->ml_patches_cap = 0;
        const size_t fl = (size_t)chunk * lg_cnn_halo_patch_floats();
        LG_HIP(h, regrow_dev(&h->ml_patches, fl));
        LG_HIP(h, hipMemset(h->ml_patches, 0, fl * sizeof(float)));   // the halos and the three spare planes stay zero
        h->ml_patches_cap = chunk;
    }
    if (want_rows && BM > h->ml_rows_cap) {
        h->ml_rows_cap = 0;
        LG_HIP(h, regrow_dev(&h->ml_rows, BM));
        h->ml_rows_cap = BM;
    }
    if (!h->ev_ml) LG_HIP(h, hipEventCreateWithFlags(&h->ev_ml, hipEventDisableTiming));
    return LG_OK;
}

// The labels entries' staging: room for the 0 / 1 mask the bit-row pass derives from the labels, the frames' leaf ids on the device
int labels_stage(lg_handle h, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W, void* stream_) {
    if (!labels || !leaf_ids || B < 1 || H < 1 || W < 1) return fail(h, LG_ERR_INVALID, "lg_select_grasp_labels: null or empty input");
    LG_HIP(h, hipSetDevice(h->device));
    const size_t need = (size_t)B * H * W;
    if (need > h->mask_ws_cap) {
        h->mask_ws_cap = 0;
        if (regrow_dev(&h->mask_ws, need) != hipSuccess) return fail(h, LG_ERR_NOMEM, "lg_select_grasp_labels: mask workspace");
        h->mask_ws_cap = need;
    }
    if (B > h->ids_cap) {
        h->ids_cap = 0;
        if (regrow_dev(&h->ids_dev, (size_t)B) != hipSuccess || regrow_pinned(&h->ids_host, (size_t)B) != hipSuccess)
            return fail(h, LG_ERR_NOMEM, "lg_select_grasp_labels: id buffers");
        h->ids_cap = B;
    }
    memcpy(h->ids_host, leaf_ids, sizeof(int32_t) * B);   // (the previous call on this handle has been synchronised: one call in flight)
    LG_HIP(h, hipMemcpyAsync(h->ids_dev, h->ids_host, sizeof(int32_t) * B, hipMemcpyHostToDevice, (hipStream_t)stream_));
    return LG_OK;
}

// candidate rows (lg_select_grasp_candidates*): on the first call that asks for them
int ensure_cand_rows(lg_ctx* h, size_t rows) {
    if (rows <= h->cand_rows_cap) return LG_OK;
    h->cand_rows_cap = 0;
    if (regrow_dev(&h->cand_rows_dev, rows) != hipSuccess || regrow_pinned(&h->cand_rows_host, rows) != hipSuccess)
        return fail(h, LG_ERR_NOMEM, "lg_select_grasp_candidates: candidate rows");
    h->cand_rows_cap = rows;
    return LG_OK;
}

// ============================================================================ the stages of a call
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
    // state byte from lg_near_tiles_kernel beside the distance transform.  Set with `sparse`, by takes_near_launch.
    bool near = false;
    // deferred planes (sparse mode, unless LG_DEFER_PLANES=0): lg_final_kernel stores what top-k reads and flatness (score-only);
    // sdf, approach, isolation, accessibility and stem are neither allocated nor written: the gather computes them at the
    // pixels of its windows
    bool defer = false;
    // label-aware mode (lg_params.label_aware, labels given): the bit-row pass also writes the other leaves' rows (iso_others)
    bool label_aware = false;
};

// label-aware mode: the workspace of the mode, on the first call that asks for it (`what`: the entry's message)
int ensure_iso_ws(lg_ctx* h, const Plan& pl, const char* what) {
    const size_t words = (size_t)pl.B * pl.H * pl.WW;
    if (words <= h->iso_words_cap && pl.B <= h->iso_B_cap) return LG_OK;
    h->iso_words_cap = 0; h->iso_B_cap = 0;
    if (regrow_dev(&h->iso_others, words) != hipSuccess || regrow_dev(&h->iso_dil, 2 * words) != hipSuccess ||
        regrow_dev(&h->iso_mf, (size_t)LG_ISO_MF * pl.B) != hipSuccess)
        return fail(h, LG_ERR_NOMEM, what);
    h->iso_words_cap = words; h->iso_B_cap = pl.B;
    return LG_OK;
}

// The workspace planes a call takes for those its caller does not want back: all eight when the CNN rescoring runs and the
// planes are not deferred (deferred: flatness, which the gather still reads); otherwise only distance + traditional.  And the
// validity plane.
int take_planes(lg_ctx* h, Plan& pl, bool use_cnn) {
    for (int i = 0; i < LG_NUM_MAPS; i++)
        if (!pl.maps[i] && ((use_cnn && (!pl.defer || i == LG_MAP_FLATNESS)) || i == LG_MAP_DISTANCE || i == LG_MAP_TRADITIONAL)) {
            const int rc = ensure_ws_map(h, i);
            if (rc) return rc;
            pl.maps[i] = h->ws_maps[i];
        }
    if (!pl.valid) pl.valid = h->ws_valid;
    return LG_OK;
}

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

// pack bits of the whole batch (h->ev_prep behind them) + what reads only the bit rows, on the side streams
int enq_prep(lg_ctx* h, const Plan& pl, hipStream_t s) {
    h->export_pending = true;
    const int n = pl.B;
    LG_HIP(h, hipMemsetAsync(h->maxfix, 0, sizeof(uint32_t) * LG_MF * n, s));
    if (pl.label_aware) LG_HIP(h, hipMemsetAsync(h->iso_mf, 0, sizeof(uint32_t) * LG_ISO_MF * n, s));
    {
        ProfScope ps(h, "prep", s);
        if (pl.labels)   // (label-aware: the other leaves' rows as well)
            lg_launch_pack_labels(pl.labels, h->ids_dev, h->mask_ws, h->bits, n, pl.H, pl.W, pl.WW, s, h->maxfix,
                                  pl.label_aware ? h->iso_others : nullptr, pl.label_aware ? h->iso_mf : nullptr);
        else
            lg_launch_pack_bits(pl.mask, h->bits, n, pl.H, pl.W, pl.WW, s, h->maxfix);
    }
    {
        ProfScope ps(h, "bbox", s);
        lg_launch_window(h->maxfix, h->win, n, pl.H, pl.W, h->opt.dt_search, s, (uint32_t)pl.P.chamfer_init_dist0);
    }
    LG_HIP(h, hipEventRecord(h->ev_prep, s));
    LG_HIP(h, hipStreamWaitEvent(h->copy_stream, h->ev_prep, 0));
    if (pl.near) {   // list offsets of the near tiles + the far tiles' keys and state bytes
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
            lg_launch_orient(h->orient, h->bits, h->win, h->fp_dev, 0, n, pl.H, pl.W, pl.WW, h->copy_stream,
                             direct ? h->fp_host_dev : nullptr);
        }
        if (!direct) {
            LG_HIP(h, hipMemcpyAsync(h->fp_host, h->fp_dev, sizeof(LgFrameParams) * n, hipMemcpyDeviceToHost, h->copy_stream));
            LG_HIP(h, hipMemcpyAsync(h->orient->h_status, h->orient->status, sizeof(int) * n, hipMemcpyDeviceToHost, h->copy_stream));
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
        if (ts != h->copy_stream) LG_HIP(h, hipStreamWaitEvent(ts, h->ev_prep, 0));
        const int rc = enq_tail(h, pl, 0, n, ts);
        if (rc) return rc;
        LG_HIP(h, hipEventRecord(h->ev_side, ts));
    }
    return LG_OK;
}

// Bit rows of the bounding boxes + the windows to the host: only for the host contour analysis (LG_HOST_ORIENT, or frames the
// device orientation kernel hands back) -- since round 3 the pre-grasp probes run on the device (lg_finish_kernel) and a normal
// call exports nothing.  The export writes pinned host memory over PCIe and slows every memory-bound kernel beside it about 4x,
// which is why it is only queued when somebody is about to wait for it.  The whole batch.
int enq_export(lg_ctx* h, const Plan& pl) {
    const size_t words = (size_t)pl.B * pl.H * pl.WW;
    if (h->bits_host_dev)   // rows of the bounding boxes only, posted writes by a small grid on the priority stream
        lg_launch_export_rows(h->bits, h->win, h->bits_host_dev, pl.B, pl.H, pl.WW, h->copy_stream);
    else
        LG_HIP(h, hipMemcpyAsync(h->bits_host, h->bits, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, h->copy_stream));
    LG_HIP(h, hipMemcpyAsync(h->win_host, h->win, sizeof(LgWin) * pl.B, hipMemcpyDeviceToHost, h->copy_stream));
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

// Label-aware mode (the whole batch; such a call is never piped): others -> two dilations -> two chamfer-3 transforms, behind the distance
// transform on the caller's stream: the fields take the sweeps' scratch (h->tmp, [B][2][H][W] words), free from here on.  A frame
// without another leaf is skipped by every kernel.
LgIsoFields iso_fields(const lg_ctx* h) { return {h->tmp, h->iso_mf}; }

int enq_iso(lg_ctx* h, const Plan& pl, hipStream_t s) {
    if (!pl.label_aware) return LG_OK;
    {
        ProfScope ps(h, "iso_dilate", s);
        lg_launch_iso_dilate(h->iso_others, h->iso_dil, h->iso_mf, pl.B, pl.H, pl.W, pl.WW, s);
    }
    {
        ProfScope ps(h, "iso_sweeps", s);
        if (lg_launch_iso_sweeps(h->iso_dil, h->tmp, h->iso_mf, pl.B, pl.H, pl.W, pl.WW, (uint32_t)pl.P.chamfer_init_dist0, s))
            return fail(h, LG_ERR_UNSUPPORTED, "label_aware: width");
    }
    return LG_OK;
}

// the stored isolation plane (dense calls, LG_DEFER_PLANES=0, the ML entries' stored form): the current leaf's pixels, behind the
// plane kernel whose arguments `fargs` are
void enq_iso_plane(lg_ctx* h, const Plan& pl, const LgFinalArgs& fargs, hipStream_t s) {
    if (!pl.label_aware || !pl.maps[LG_MAP_ISOLATION]) return;
    ProfScope ps(h, "iso_plane", s);
    lg_launch_iso_plane(iso_fields(h), h->bits, h->win, pl.maps[LG_MAP_ISOLATION], pl.B, pl.H, pl.W, pl.WW, pl.P.iso_w_close,
                        pl.P.iso_w_wide, fargs.iso_ramp_top, fargs.iso_ramp_step, s);
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

// Orientation of every frame into fp_host (and fp_dev).  Device path: wait for lg_orient_kernel's results (it runs
// beside the sweeps on the side stream); frames it handed back (status 1: more runs than its scratch holds) are analysed on
// the host threads.  LG_HOST_ORIENT: every frame on the host.  *upload = fp_host has entries the device does not have yet.
int finish_orient(lg_ctx* h, const Plan& pl, bool* upload) {
    *upload = true;
    h->last_redo = 0;
    if (!h->orient) {
        if (h->export_pending) { const int rc = enq_export(h, pl); if (rc) return rc; }
        LG_HIP(h, hipEventSynchronize(h->ev_copy));   // bit rows are on the host; the sweeps are running
        parallel_for(h, pl.B, [=, &pl](int b) { host_orient_frame(h, pl, b); });
        return LG_OK;
    }
    LG_HIP(h, hipEventSynchronize(h->ev_orient));
    std::vector<int> redo;
    for (int b = 0; b < pl.B; b++)
        if (h->orient->h_status[b]) redo.push_back(b);
    h->last_redo = (int)redo.size();
    *upload = !redo.empty();
    if (redo.empty()) return LG_OK;
    if (h->export_pending) { const int rc = enq_export(h, pl); if (rc) return rc; }
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
    if (pl.near) {   // (the whole batch, or one lane of its tail: the entries of the batch's list that the frames [off, off + n) own)
        LG_HIP(h, hipEventSynchronize(h->ev_near));   // near_off_host is written (the kernel ended long ago: it follows the bit-row pass)
        a.near_off = h->near_off + off;
        a.near_base = h->near_off_host[off];
        a.near_total = h->near_off_host[off + n] - h->near_off_host[off];
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
              float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid) {
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
    // a real distance must stay below the sweeps' "no path" value wherever OpenCV's border cells do not hide it (lg_dt_far)
    if (lg_norm5(W - 1, H - 1) + 2u * LG_C5 >= LG_INF && (uint32_t)pl.P.chamfer_init_dist0 > LG_NOSRC)
        return fail(h, LG_ERR_UNSUPPORTED, "chamfer_init_dist0 above INT_MAX >> 2 needs a frame whose diagonal stays below 16384 px");
    if (lg_label_aware_check(&pl.P, 1)) return fail(h, LG_ERR_INVALID, "label_aware must be 0 or 1");
    pl.B = B; pl.H = H; pl.W = W; pl.WW = (W + 63) / 64;
    pl.tiles_x = (W + LG_TW - 1) / LG_TW; pl.tiles_y = (H + LG_TH - 1) / LG_TH;
    if (pl.tiles_x * pl.tiles_y > 8192) return fail(h, LG_ERR_UNSUPPORTED, "image too large for the top-k tile table");
    pl.depth = depth; pl.mask = mask; pl.valid = out_valid;
    for (int i = 0; i < LG_NUM_MAPS; i++) pl.maps[i] = out_maps ? out_maps[i] : nullptr;
    return LG_OK;
}

// LG_TRACE: the host's stamps of a call's stages and, for a call that is not piped, the device's timeline on the caller's stream
struct Timeline {
    enum { START, ENQ1, ORIENT, ENQ2, SYNC, SWEEPS = 1, PLANES, TOPK, CNN };   // host stamps; events on the stream
    const bool on, gpu;
    const hipStream_t s;
    double t[5] = {0};
    hipEvent_t ev[5] = {nullptr};
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    Timeline(bool on_, bool gpu_, hipStream_t s_) : on(on_), gpu(on_ && gpu_), s(s_) {
        if (!on) return;
        t[START] = now();
        for (auto& e : ev) hipEventCreate(&e);
        hipEventRecord(ev[START], s);
    }
    ~Timeline() { for (auto e : ev) if (e) hipEventDestroy(e); }
    void host(int i) { if (on) t[i] = now(); }
    void mark(int i) { if (gpu) hipEventRecord(ev[i], s); }
    void print(int B) {   // after the call's synchronise (tools/trace_run.py reads both lines)
        if (!on) return;
        if (gpu) {
            float a[5] = {0};
            for (int i = 1; i <= 4; i++) hipEventElapsedTime(&a[i], ev[START], ev[i]);
            fprintf(stderr, "[lg] gpu timeline (ms since call start): sweeps done %.3f | planes %.3f | topk %.3f | cnn %.3f\n", a[1], a[2],
                    a[3], a[4]);
        }
        // (the host has not waited for the bit rows since the orientation moved to the device: that field stays, at zero)
        fprintf(stderr, "[lg] B=%d enq1 %.3f | wait bits %.3f | orient %.3f | enq2 %.3f | gpu wait %.3f | post %.3f ms\n", B,
                t[ENQ1] - t[START], 0.0, t[ORIENT] - t[ENQ1], t[ENQ2] - t[ORIENT], t[SYNC] - t[ENQ2], now() - t[SYNC]);
    }
};

// Plan::near: does a call with this plan take the near launch of the plane kernel?  Asked once per call, where `sparse` is set
// (an LG_SUBBATCH handle never does: its plane launches are per sub-batch, the list is the batch's).
bool takes_near_launch(const lg_ctx* h, const Plan& pl) {
    return pl.sparse && h->opt.final_near > 0 && h->opt.subbatch == 0 && h->opt.no_skip == 0;
}

// enq_front up to, and without, the plane kernel.  *upload_fp: as finish_orient's.
template <typename AfterPrep>
int enq_front_sweeps(lg_ctx* h, const Plan& pl, hipStream_t s, Timeline* tl, AfterPrep&& after_prep, bool* upload_fp) {
    int rc = enq_prep(h, pl, s);
    if (rc) return rc;
    if ((rc = after_prep())) return rc;
    if ((rc = enq_dt(h, pl, 0, pl.B, s))) return rc;
    if ((rc = enq_iso(h, pl, s))) return rc;
    if (tl) { tl->mark(Timeline::SWEEPS); tl->host(Timeline::ENQ1); }
    if ((rc = finish_orient(h, pl, upload_fp))) return rc;   // theta per frame: device results (or host analysis) while the sweeps run
    if (tl) tl->host(Timeline::ORIENT);
    return LG_OK;
}

// A whole call on the caller's stream, up to its planes: bit rows -> `after_prep` (what else reads only the bit rows and the
// bounding boxes) -> distance transform -> label-aware fields -> orientation -> plane kernel -> stored isolation plane.
// *fargs: the plane launch's arguments, for the deferred gather.
template <typename AfterPrep>
int enq_front(lg_ctx* h, const Plan& pl, hipStream_t s, LgFinalArgs* fargs, AfterPrep&& after_prep) {
    bool upload_fp = true;
    int rc = enq_front_sweeps(h, pl, s, nullptr, after_prep, &upload_fp);
    if (rc) return rc;
    if ((rc = enq_final(h, pl, 0, pl.B, s, upload_fp, fargs))) return rc;
    enq_iso_plane(h, pl, *fargs, s);
    return LG_OK;
}
int nothing_after_prep() { return LG_OK; }

// lg_finish_kernel's arguments, but for the candidate list, its logits and slots, which the caller sets
LgFinishArgs finish_args(lg_ctx* h, const Plan& pl, int K, bool use_cnn) {
    LgFinishArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.bits2 = pl.label_aware ? h->iso_others : nullptr;
    fa.fp = h->fp_dev; fa.bits = h->bits; fa.out = h->res_host_dev ? h->res_host_dev : h->res_dev;
    fa.B = pl.B; fa.H = pl.H; fa.W = pl.W; fa.WW = pl.WW; fa.K = K; fa.use_cnn = use_cnn ? 1 : 0; fa.mask_is_bool = pl.P.mask_is_bool;
    fa.cx = pl.P.cx; fa.cy = pl.P.cy; fa.f = pl.P.f;
    lg_make_se_spans(2 * pl.P.pregrasp_clearance + 1, &fa.se);
    return fa;
}

// The end of a call: its B result rows come back (`who`: the entry, for its message); what else comes back on `s` is queued already
int return_results(lg_ctx* h, const Plan& pl, lg_grasp_result* results, bool use_cnn, const char* who, hipStream_t s, Timeline* tl = nullptr) {
    // (with a device alias lg_finish_kernel wrote the rows into res_host itself: they are there behind the synchronise below)
    if (!h->res_host_dev)
        LG_HIP(h, hipMemcpyAsync(h->res_host, h->res_dev, sizeof(lg_grasp_result) * pl.B, hipMemcpyDeviceToHost, s));
    if (tl) tl->host(Timeline::ENQ2);
    LG_HIP(h, hipStreamSynchronize(s));
    if (tl) tl->host(Timeline::SYNC);
    LG_HIP(h, hipGetLastError());
    if (use_cnn && lg_cnn_take_error(&h->cnn))
        return fail(h, LG_ERR_HIP, (std::string(who) + ": a split CNN item did not receive its parts").c_str());
    memcpy(results, h->res_host, sizeof(lg_grasp_result) * pl.B);
    if (pl.near) h->last_near_B = pl.B;
    if (pl.label_aware) { h->last_iso_B = pl.B; h->last_iso_H = pl.H; h->last_iso_W = pl.W; }
    return LG_OK;
}

// ============================================================================ the tail of lg_select_grasp*, per frame range
// What the ranges of one call's tail share, and range k of it -- a lane, or a sub-batch: frames [off, off + n), with the first
// pixel of its planes, the first tile of its tile tables and the first of its K-per-frame candidate slots.
struct Tail {
    lg_ctx* h; const Plan& pl; int K; bool use_cnn, prune;
    std::vector<LgFinalArgs> fargs;   // per range: the plane launch's arguments, for the deferred gather
    LgIsoFields iso;
};
struct Range { int k, off, n; size_t px, tile, cand; };
Range frame_range(const Tail& t, int SB, int k) {
    const Plan& pl = t.pl;
    const int off = k * SB;
    return {k, off, std::min(SB, pl.B - off), (size_t)off * pl.H * pl.W, (size_t)off * pl.tiles_x * pl.tiles_y, (size_t)off * t.K};
}

// The untimed events of range k (h->ev_pool): its sweeps, its planes, its top-k are queued; it has ended.
enum { EV_DT, EV_PLANES, EV_TOPK, EV_DONE, EV_PER_RANGE };
hipEvent_t range_ev(const lg_ctx* h, int k, int which) { return h->ev_pool[EV_PER_RANGE * k + which]; }
int ensure_range_events(lg_ctx* h, int ranges) {
    while ((int)h->ev_pool.size() < EV_PER_RANGE * ranges) {
        hipEvent_t e;
        LG_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ev_pool.push_back(e);
    }
    return LG_OK;
}

// greedy spaced top-k of the range's frames and, pruned, the candidates of each that can still win (surv_keep)
void enq_topk(const Tail& t, const Range& r, hipStream_t s) {
    lg_ctx* h = t.h; const Plan& pl = t.pl;
    const lg_params& P = pl.P;
    ProfScope ps(h, "topk", s);
    lg_launch_topk(pl.maps[LG_MAP_TRADITIONAL] + r.px, pl.valid + r.px, pl.depth + r.px, h->tilekeys + r.tile,
                   pl.sparse ? h->tile_state + r.tile : nullptr, P.flat_scale, P.w_flat, true, r.n, pl.H, pl.W, t.K, P.nms_min_distance,
                   h->cand_xy + r.cand * 2, h->cand_n + r.off, h->cand_info + r.cand * 2, s, t.prune ? h->surv_keep + r.off : nullptr,
                   P.mask_is_bool);
}

// CNN rescoring of the range's candidates, behind its top-k on `s`: survivors (pruned: the range's own list, slot map and count)
// -> patch gather -> lg_cnn_run on the activation buffers from slot act_off on.  Without a model: nothing.
int enq_rescore(const Tail& t, const Range& r, hipStream_t s, int act_off) {
    if (!t.use_cnn) return LG_OK;
    lg_ctx* h = t.h; const Plan& pl = t.pl;
    const int32_t* list = t.prune ? h->surv_list + r.cand : nullptr;
    const int32_t* count = t.prune ? h->surv_count + r.k : nullptr;
    float* patches = h->patches + r.cand * lg_cnn_halo_patch_floats();
    if (t.prune) {
        ProfScope ps(h, "survivors", s);
        lg_launch_survivors(h->surv_keep + r.off, r.n, t.K, h->surv_list + r.cand, h->surv_slot + r.cand, h->surv_count + r.k, s);
    }
    {
        ProfScope ps(h, "gather", s);
        const float* mp[LG_NUM_MAPS];
        for (int i = 0; i < LG_NUM_MAPS; i++) mp[i] = pl.maps[i] ? pl.maps[i] + r.px : nullptr;
        lg_launch_gather(pl.depth + r.px, pl.mask + r.px, mp, pl.sparse ? h->tile_state + r.tile : nullptr, pl.P.flat_scale, r.n, pl.H,
                         pl.W, t.K, h->cand_xy + r.cand * 2, h->cand_n + r.off, patches, true, s, list, count,
                         pl.defer ? &t.fargs[r.k] : nullptr, pl.label_aware ? &t.iso : nullptr);
    }
    std::string err;
    ProfScope ps(h, "cnn", s);
    const int rc = lg_cnn_run(&h->cnn, patches, true, r.n * t.K, h->logits + r.cand, s, &err, false, count, act_off);
    return rc ? fail(h, rc, err.c_str()) : LG_OK;
}

// ============================================================================ how a call's frames are cut, and its two schedules
// One range -- the ordinary call --, tail lanes, or the sub-batches of an LG_SUBBATCH handle (label-aware calls excepted: their
// transforms reuse the sweeps' scratch).  `ranges` ranges of SB frames, the last one shorter; lane_slots: a lane's range of the
// CNN's activation buffers.
// Lanes run only where the pruned CNN pass follows the near launch: a model, LG_CNN_PRUNE, not the candidates entry, not
// label-aware, not piped (lg_tail_lane_plan has the rule, lg_debug_tail_lanes overrides it; DESIGN.md section 4, "Tail in lanes").
// The automatic rule also asks that no other handle of the process is inside a selection call (InFlight, which lives as long as
// the call): lanes fill the holes of a chip this call would otherwise have to itself.  With two batches in flight on two
// handles (bench.py's `pipelined`) the other batch fills them already, and lanes cost 5-10 % there (1.74, 1.82 against 1.65,
// 1.67 ms per step before this rule).  Results never depend on the lanes, so a rule that depends on timing is safe.
// And it asks that the call's B * K patch slots fit one slice of lg_cnn_run: a larger call runs its CNN in slices one behind
// the other in the activation workspace of ONE slice (6.5 GB for the standard model); in lanes each lane would hold a slice's
// worth of it.  The automatic rule never grows that workspace beyond what the one-lane call takes.  A forced setting ignores both.
struct InFlight {
    const int others;
    InFlight() : others(g_select_in_flight.fetch_add(1, std::memory_order_relaxed)) {}
    ~InFlight() { g_select_in_flight.fetch_sub(1, std::memory_order_relaxed); }
};
struct Cut { bool piped; int lanes, SB, ranges, lane_slots; };
Cut cut_frames(const lg_ctx* h, const Plan& pl, int K, bool prune, const InFlight& in_flight) {
    const int B = pl.B;
    Cut c = {false, 1, B, 1, 0};
    if (h->opt.subbatch > 0 && !pl.label_aware) c.SB = h->opt.subbatch;
    c.piped = c.SB < B;
    const bool one_slice = lg_cnn_act_slots(B * K) == B * K;
    const int lanes_req = h->tail_lanes_req ? h->tail_lanes_req : (in_flight.others || !one_slice ? 1 : 0);
    int32_t lanes = 1, lane_sb = B;
    lg_tail_lane_plan(B, lanes_req, !c.piped && prune && !pl.label_aware && pl.near, &lanes, &lane_sb);
    if (lanes > 1) { c.lanes = lanes; c.SB = lane_sb; }
    c.ranges = (B + c.SB - 1) / c.SB;
    c.lane_slots = lg_cnn_act_slots(c.SB * K);
    return c;
}

// The call in lanes; one lane is the ordinary call.  The front runs ONCE for the whole batch and only what follows it -- planes,
// top-k, survivors, gather, CNN -- runs per lane of SB consecutive frames, each lane an in-order chain on a stream of its own:
// lane 0 on the caller's, lanes 1 .. on library streams that are idle by now (s_main first: LG_TAIL_LANE_STREAMS has the
// reading), lane k's plane launch behind lane k - 1's, which puts it behind the front and staggers the lanes; the caller's
// stream goes on behind every lane.  The front costs what it did and the lanes fill each other's holes: the left-over rounds
// of a lane's persistent CNN launches, its seven launch boundaries and its one-workgroup-per-frame top-k run beside the other
// lane's matrix work (1.82 against 1.89 ms per step at 256 frames).  Whole CNN items, a survivor list, count and slot map per
// lane and a range of the activation buffers per lane (lg_cnn_run's act_off; room reserved by the caller before anything is
// queued) keep every logit, candidate and result row equal to the one-lane call's bit for bit.
// One lane: everything on the caller's stream, no event, prof_cont never set.  The timeline's marks follow lane 0.
int schedule_lanes(Tail& t, const Cut& c, hipStream_t s, Timeline& tl) {
    lg_ctx* h = t.h; const Plan& pl = t.pl;
    bool upload_fp = true;
    int rc = enq_front_sweeps(h, pl, s, &tl, nothing_after_prep, &upload_fp);
    if (rc) return rc;
    const hipStream_t lane_s[4] = {s, LG_TAIL_LANE_STREAMS};
    for (int k = 0; k < c.lanes; k++) {
        const Range r = frame_range(t, c.SB, k);
        const hipStream_t ls = lane_s[k];
        h->prof_cont = k > 0;
        if (k) LG_HIP(h, hipStreamWaitEvent(ls, range_ev(h, k - 1, EV_PLANES), 0));
        if ((rc = enq_final(h, pl, r.off, r.n, ls, upload_fp, &t.fargs[k]))) return rc;
        if (k + 1 < c.lanes) LG_HIP(h, hipEventRecord(range_ev(h, k, EV_PLANES), ls));
        enq_iso_plane(h, pl, t.fargs[k], ls);   // (the whole batch's: label-aware calls are one lane)
        if (!k) tl.mark(Timeline::PLANES);
        enq_topk(t, r, ls);
        if (!k) tl.mark(Timeline::TOPK);
        if ((rc = enq_rescore(t, r, ls, k * c.lane_slots))) return rc;
        if (k) LG_HIP(h, hipEventRecord(range_ev(h, k, EV_DONE), ls));
    }
    h->prof_cont = false;
    for (int k = 1; k < c.lanes; k++) LG_HIP(h, hipStreamWaitEvent(s, range_ev(h, k, EV_DONE), 0));
    tl.mark(Timeline::CNN);
    return LG_OK;
}

// The LG_SUBBATCH experiment (LG_SUBBATCH=n in the environment when the handle is created): the front is cut as well.  Stages
// per sub-batch k of SB frames:
//   D(k): distance sweeps (the bit rows: once, in front)   -- latency bound, 2*SB workgroups  -> s_dt[k&1]
//   F(k): fused score planes                               -- HBM bound                       -> s_main
//   T(k): greedy spaced top-k                              -- latency bound, SB workgroups    -> s_topk
//   G(k): survivors, patch gather, CNN                     -- MFMA bound                      -> s_main
// s_main runs F(0) F(1) G(0) F(2) G(1) ... so T(k) hides behind F(k+1) and the D chain behind everything.
// Measured on MI355X (B=128, 1080p): SB=32 is 14.8 ms/step vs 11.5 ms in one range -- the chain D(0)->F(0)->T(0) must drain
// before the first CNN launch, and D's latency does not shrink with SB.  The lanes above cut only the tail, and win.
int schedule_subbatches(Tail& t, const Cut& c, hipStream_t s, Timeline& tl) {
    lg_ctx* h = t.h; const Plan& pl = t.pl;
    const hipStream_t sD[2] = {h->s_dt[0], h->s_dt[1]}, sM = h->s_main, sT = h->s_topk;
    // internal streams start after whatever the caller queued on `s`
    LG_HIP(h, hipEventRecord(h->ev_begin, s));
    for (hipStream_t q : {sD[0], sD[1], sM, sT}) LG_HIP(h, hipStreamWaitEvent(q, h->ev_begin, 0));
    // bit rows of the whole batch first (one short kernel) so the host never waits behind a distance sweep
    int rc = enq_prep(h, pl, sD[0]);
    if (rc) return rc;
    LG_HIP(h, hipStreamWaitEvent(sD[1], h->ev_prep, 0));
    for (int k = 0; k < c.ranges; k++) {
        const Range r = frame_range(t, c.SB, k);
        if ((rc = enq_dt(h, pl, r.off, r.n, sD[k & 1]))) return rc;
        LG_HIP(h, hipEventRecord(range_ev(h, k, EV_DT), sD[k & 1]));
    }
    tl.host(Timeline::ENQ1);
    bool upload_fp = true;
    if ((rc = finish_orient(h, pl, &upload_fp))) return rc;
    tl.host(Timeline::ORIENT);
    for (int k = 0; k < c.ranges; k++) {   // F(k) T(k) G(k - 1)
        const Range r = frame_range(t, c.SB, k);
        LG_HIP(h, hipStreamWaitEvent(sM, range_ev(h, k, EV_DT), 0));
        if ((rc = enq_final(h, pl, r.off, r.n, sM, upload_fp, &t.fargs[k]))) return rc;
        LG_HIP(h, hipEventRecord(range_ev(h, k, EV_PLANES), sM));
        LG_HIP(h, hipStreamWaitEvent(sT, range_ev(h, k, EV_PLANES), 0));
        enq_topk(t, r, sT);
        LG_HIP(h, hipEventRecord(range_ev(h, k, EV_TOPK), sT));
        if (k >= 1) {
            LG_HIP(h, hipStreamWaitEvent(sM, range_ev(h, k - 1, EV_TOPK), 0));
            if ((rc = enq_rescore(t, frame_range(t, c.SB, k - 1), sM, 0))) return rc;
        }
    }
    LG_HIP(h, hipStreamWaitEvent(sM, range_ev(h, c.ranges - 1, EV_TOPK), 0));
    if ((rc = enq_rescore(t, frame_range(t, c.SB, c.ranges - 1), sM, 0))) return rc;
    for (hipStream_t q : {sD[0], sD[1], sM, sT}) {   // join: the caller's stream continues after every internal stream
        LG_HIP(h, hipEventRecord(range_ev(h, 0, EV_DONE), q));
        LG_HIP(h, hipStreamWaitEvent(s, range_ev(h, 0, EV_DONE), 0));
        LG_HIP(h, hipStreamSynchronize(q));
    }
    return LG_OK;
}

int lg_select_grasp_impl(lg_handle h, const float* depth, const uint8_t* mask, const int16_t* labels, int B, int H, int W,
                         const lg_params* pin, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, lg_grasp_result* results,
                         lg_grasp_candidate* cands, void* stream_) {
    if (!results) return fail(h, LG_ERR_INVALID, "lg_select_grasp: results is null");
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, out_maps, out_valid);
    if (rc) return rc;
    pl.labels = labels;
    if (lg_label_aware_check(&pl.P, labels ? 1 : 0))
        return fail(h, LG_ERR_INVALID, "lg_select_grasp: label_aware needs the label image (lg_select_grasp_labels, lg_select_grasp_candidates_labels)");
    pl.label_aware = pl.P.label_aware != 0;
    pl.sparse = !out_valid;
    for (int i = 0; i < LG_NUM_MAPS; i++) pl.sparse = pl.sparse && !pl.maps[i];
    pl.near = takes_near_launch(h, pl);
    pl.defer = pl.sparse && h->opt.defer_planes;
    const int K = pl.P.top_k;
    if (K < 1 || K > 64) return fail(h, LG_ERR_INVALID, "lg_select_grasp: top_k must be in [1,64]");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure_ws(h, B, H, W, K))) return rc;
    reset_last(h);
    if (pl.label_aware) rc = ensure_iso_ws(h, pl, "lg_select_grasp_labels: label-aware workspace");
    if (!rc && cands) rc = ensure_cand_rows(h, (size_t)B * K);
    if (rc) return rc;
    const bool use_cnn = h->cnn.loaded;
    // The CNN on the candidates that can still win only (the result row needs no other; the candidates entry reports an ML
    // score for every candidate and scores them all).  Either way no item of the CNN is split: a patch's logit then does not
    // depend on how many patches run beside it, and the rows of both entries, pruned or not, are equal bit for bit.
    const bool prune = use_cnn && !cands && h->opt.cnn_prune && lg_cnn_counts_on_device(&h->cnn);
    if (use_cnn) h->last_scored = (long long)B * K;
    if ((rc = take_planes(h, pl, use_cnn))) return rc;
    InFlight in_flight;
    const Cut c = cut_frames(h, pl, K, prune, in_flight);
    h->last_tail_lanes = c.lanes;
    if (c.lanes > 1) {   // the lanes' ranges of the CNN's activation buffers: made before anything is queued (growing them synchronises and frees)
        std::string err;
        const int r2 = lg_cnn_reserve(&h->cnn, (c.lanes - 1) * c.lane_slots + lg_cnn_act_slots((B - (c.lanes - 1) * c.SB) * K), s, &err);
        if (r2) return fail(h, r2, err.c_str());
    }
    if ((rc = ensure_range_events(h, c.ranges))) return rc;
    struct ContGuard { lg_ctx* h; ~ContGuard() { h->prof_cont = false; } } cont_guard{h};
    Tail t{h, pl, K, use_cnn, prune, std::vector<LgFinalArgs>((size_t)c.ranges), iso_fields(h)};
    Timeline tl(h->opt.trace, !c.piped, s);
    if ((rc = c.piped ? schedule_subbatches(t, c, s, tl) : schedule_lanes(t, c, s, tl))) return rc;
    if (prune) h->last_scored_subs = c.ranges;
    // ---- the rest of select_grasp_point per frame -- rescoring, 3-D point, pre-grasp probes -- on the device (lg_finish_kernel);
    //      one copy of B result rows comes back
    {
        LgFinishArgs fa = finish_args(h, pl, K, use_cnn);
        fa.cand_n = h->cand_n; fa.cand_xy = h->cand_xy; fa.cand_info = h->cand_info; fa.logits = h->logits;
        fa.slot = prune ? h->surv_slot : nullptr; fa.slot_frames = c.SB;
        {
            ProfScope ps(h, "finish", s);
            lg_launch_finish(fa, s);
        }
        if (cands) {
            ProfScope ps(h, "candidates", s);
            lg_launch_candidates(fa, h->cand_rows_dev, s);
        }
    }
    if (cands)
        LG_HIP(h, hipMemcpyAsync(h->cand_rows_host, h->cand_rows_dev, sizeof(lg_grasp_candidate) * B * K, hipMemcpyDeviceToHost, s));
    if ((rc = return_results(h, pl, results, use_cnn, "lg_select_grasp", s, &tl))) return rc;
    if (cands) memcpy(cands, h->cand_rows_host, sizeof(lg_grasp_candidate) * B * K);
    if (use_cnn) { h->last_cnn_B = B; h->last_cnn_K = K; h->last_cnn_SB = c.SB; h->last_cnn_pruned = prune; }
    h->last_patch_floats = use_cnn ? (long long)B * K * lg_cnn_halo_patch_floats() : 0;
    tl.print(B);
    return LG_OK;
}

// ML-only grasp selection (lg_mlsel.h): the front without top-k; then the sample table's scored windows through the gather and the
// CNN in chunks, the pick, lg_finish_kernel on the one-point list.
int lg_select_grasp_ml_impl(lg_handle h, const float* depth, const uint8_t* mask, const int16_t* labels, int B, int H, int W,
                            const lg_params* pin, const lg_ml_sampling* sp, lg_grasp_result* results, lg_ml_sample* samples,
                            int32_t* n_samples, void* stream_) {
    if (!results) return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: results is null");
    lg_ml_sampling S;
    if (sp) S = *sp; else lg_default_ml_sampling(&S);
    if (const char* why = lg_ml_sampling_error(&S)) return fail(h, LG_ERR_INVALID, (std::string("lg_select_grasp_ml: ") + why).c_str());
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, nullptr, nullptr);
    if (rc) return rc;
    pl.labels = labels;
    if (lg_label_aware_check(&pl.P, labels ? 1 : 0))
        return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: label_aware needs the label image (lg_select_grasp_ml_labels)");
    if ((size_t)B * S.max_samples > 0x7fffffffull) return fail(h, LG_ERR_INVALID, "lg_select_grasp_ml: B * max_samples must stay below 2^31");
    pl.label_aware = pl.P.label_aware != 0;
    pl.sparse = true;
    pl.near = takes_near_launch(h, pl);
    const lg_params& P = pl.P;
    const int M = S.max_samples, chunk = S.chunk > 0 ? S.chunk : LG_ML_DEFAULT_CHUNK;
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure_ws(h, B, H, W, std::max(P.top_k, 1)))) return rc;
    if ((rc = ml_ensure(h, B, H, M, chunk, samples != nullptr))) return rc;
    reset_last(h);
    if (pl.label_aware) rc = ensure_iso_ws(h, pl, "lg_select_grasp_ml_labels: label-aware workspace");
    if (rc) return rc;
    const bool use_cnn = h->cnn.loaded;
    // Where the gather finds sdf, approach, isolation, accessibility and stem: computed at every window's pixels (deferred), or
    // stored once by the plane kernel on the leaf's tiles.  Overlapping GRID windows recompute a pixel up to (32 / stride)^2
    // times in the deferred form, yet at 1080p the gather takes the same time either way (GRID / 8, 32 frames, 46296 windows:
    // 1.265 against 1.269 ms; NTH / 100: 0.108 against 0.111) and the score-only plane kernel is the cheaper one (0.034 against
    // 0.046 ms): deferred always, which also keeps five planes out of the workspace (profiles/NOTES_ml_select.md).
    const int form = h->ml_planes ? h->ml_planes : h->opt.defer_planes ? 1 : 2;
    pl.defer = form == 1;
    h->ml_last_form = form;
    if ((rc = take_planes(h, pl, use_cnn))) return rc;
    const LgMlBuffers& m = h->ml;
    LgFinalArgs fargs;
    // the table needs the bit rows and the bounding boxes only: it runs in front of the distance transform and the host reads
    // its counts behind ev_ml, after everything up to the plane kernel has been queued
    rc = enq_front(h, pl, s, &fargs, [&]() -> int {
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
        return LG_OK;
    });
    if (rc) return rc;
    LG_HIP(h, hipEventSynchronize(h->ev_ml));   // (the table kernels ended long ago: they follow the bit-row pass)
    long long total = 0;
    for (int b = 0; b < B; b++) total += h->ml_counts_host[2 * b + 1];
    if (use_cnn && total > 0) {
        const int n_chunks = (int)((total + chunk - 1) / chunk);
        for (int c = 0; c < n_chunks; c++) h->ml_chunk_host[c] = (int32_t)std::min<long long>(chunk, total - (long long)c * chunk);
        LG_HIP(h, hipMemcpyAsync(h->ml_chunk_dev, h->ml_chunk_host, sizeof(int32_t) * n_chunks, hipMemcpyHostToDevice, s));
        const LgIsoFields iso = iso_fields(h);
        const float* mp[LG_NUM_MAPS];
        for (int i = 0; i < LG_NUM_MAPS; i++) mp[i] = pl.maps[i];
        for (int c = 0; c < n_chunks; c++) {
            const int nc = h->ml_chunk_host[c];
            {
                // patch slot j of the pass takes list entry c * chunk + j = frame * M + sample; the grid covers nc slots
                ProfScope ps(h, "gather", s);
                lg_launch_gather(depth, mask, mp, h->tile_state, P.flat_scale, (nc + M - 1) / M, H, W, M, m.xy, m.n_frame, h->ml_patches,
                                 true, s, m.list + (size_t)c * chunk, h->ml_chunk_dev + c, pl.defer ? &fargs : nullptr,
                                 pl.label_aware && pl.defer ? &iso : nullptr);
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
    LgFinishArgs fa = finish_args(h, pl, 1, false);   // the one-point list: nothing to rescore
    fa.cand_n = m.pick_n; fa.cand_xy = m.pick_xy; fa.cand_info = m.pick_info; fa.slot_frames = B;
    {
        ProfScope ps(h, "finish", s);
        lg_launch_finish(fa, s);
    }
    {
        ProfScope ps(h, "ml_rows_out", s);
        lg_launch_ml_rows_out(m, M, B, use_cnn ? 1 : 0, fa.out, samples ? h->ml_rows : nullptr, s);
    }
    if (samples) LG_HIP(h, hipMemcpyAsync(samples, h->ml_rows, sizeof(lg_ml_sample) * (size_t)B * M, hipMemcpyDeviceToHost, s));
    if ((rc = return_results(h, pl, results, use_cnn, "lg_select_grasp_ml", s))) return rc;
    if (n_samples)
        for (int b = 0; b < B; b++) n_samples[b] = h->ml_counts_host[2 * b];
    return LG_OK;
}

// ============================================================================ the collecting selector (lg_collect.h)
// why the two parameter structs are refused (null: they are not), and with which status
const char* collect_params_error(const lg_params* p, const lg_collect_params* cp, int* code) {
    lg_collect_params d;
    if (!cp) { lg_default_collect_params(&d); cp = &d; }
    *code = LG_ERR_INVALID;
    if (p && p->label_aware != 0) return "label_aware must be 0 (the collecting selector takes one mask, no label image)";
    if (cp->tip_aware != 0 && cp->tip_aware != 1) return "tip_aware must be 0 or 1";
    *code = LG_ERR_UNSUPPORTED;
    if (cp->erosion_kernel_size < 1 || cp->erosion_kernel_size > 63 || !(cp->erosion_kernel_size & 1))
        return "erosion_kernel_size must be odd and in [1,63]";
    if (cp->erosion_iterations < 0 || cp->erosion_iterations > 8) return "erosion_iterations must be in [0,8]";
    if (cp->tip_aware == 1) {
        if (cp->tip_se < 3 || cp->tip_se > 63 || !(cp->tip_se & 1)) return "tip_se must be odd and in [3,63]";
        return "tip_aware = 1 is not built (the tip penalty as written, tip_aware = 0, is)";
    }
    *code = LG_OK;
    return nullptr;
}

// safe = erode(mask, ellipse k, iterations) as 0 / 1 bytes, from the mask's bit rows (h->bits) and bounding boxes (h->win); sums:
// the original mask's centroid numerators into the workspace as well
void enq_erode(lg_ctx* h, int B, int H, int W, int WW, int k, int iterations, uint8_t* safe, bool sums, hipStream_t s) {
    LgColWs& c = h->col;
    ProfScope ps(h, "col_erode", s);
    if (sums) hipMemsetAsync(c.sums, 0, sizeof(unsigned long long) * LG_COL_SUMS * B, s);
    lg_launch_col_complement(h->bits, c.comp[0], sums ? c.sums : nullptr, B, H, W, WW, s);
    for (int i = 0; i < iterations; i++) lg_launch_col_erode_step(c.comp[i & 1], c.comp[(i + 1) & 1], h->win, B, H, W, WW, k, s);
    lg_launch_col_unpack(c.comp[iterations & 1], safe, B, H, W, WW, s);
}

// Two passes of the front: flatness alone on the original mask (a whole-frame plane, bkp:88-89), everything else on `safe`, whose
// bit rows, bounding boxes and angles the handle then holds for the tail.  The erosion runs behind the first pass's bit rows.
int lg_select_grasp_collect_impl(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                                 const lg_collect_params* cpin, float* const out_maps[LG_NUM_MAPS], float* out_tip, uint8_t* out_safe,
                                 uint8_t* out_valid, lg_grasp_result* results, void* stream_) {
    if (!results) return fail(h, LG_ERR_INVALID, "lg_select_grasp_collect: results is null");
    lg_collect_params CP;
    if (cpin) CP = *cpin; else lg_default_collect_params(&CP);
    Plan po;   // the original mask: flatness
    int rc = make_plan(h, po, depth, mask, B, H, W, pin, nullptr, nullptr);
    if (rc) return rc;
    if (const char* why = collect_params_error(&po.P, &CP, &rc)) return fail(h, rc, (std::string("lg_select_grasp_collect: ") + why).c_str());
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure_ws(h, B, H, W, 20))) return rc;
    if ((rc = col_ensure(h, B, H, W))) return rc;
    reset_last(h);
    LgColWs& c = h->col;
    float* planes[LG_NUM_MAPS + 1];   // the caller's, or the workspace's for those the fusion reads; [8]: tip
    for (int i = 0; i <= LG_NUM_MAPS; i++) {
        planes[i] = i < LG_NUM_MAPS ? (out_maps ? out_maps[i] : nullptr) : out_tip;
        if (!planes[i] && i != LG_MAP_ISOLATION && i != LG_MAP_ACCESS && (rc = col_plane(h, i, &planes[i]))) return rc;
    }
    uint8_t* safe = out_safe ? out_safe : c.safe;
    po.maps[LG_MAP_FLATNESS] = planes[LG_MAP_FLATNESS];
    if ((rc = take_planes(h, po, false))) return rc;
    LgFinalArgs fargs;
    rc = enq_front(h, po, s, &fargs, [&]() -> int {
        enq_erode(h, B, H, W, po.WW, CP.erosion_kernel_size, CP.erosion_iterations, safe, true, s);
        return LG_OK;
    });
    if (rc) return rc;
    Plan ps;   // the eroded mask: every other plane, the angle, the bit rows of the pre-grasp probes
    if ((rc = make_plan(h, ps, depth, safe, B, H, W, pin, nullptr, out_valid))) return rc;
    for (int i = 0; i < LG_NUM_MAPS; i++) ps.maps[i] = i == LG_MAP_FLATNESS ? nullptr : planes[i];
    if (!ps.valid) ps.valid = h->ws_valid;
    if ((rc = enq_front(h, ps, s, &fargs, nothing_after_prep))) return rc;
    {
        ProfScope pf(h, "col_tip", s);
        lg_launch_col_tip(safe, planes[LG_NUM_MAPS], B, H, W, (uint32_t)ps.P.chamfer_init_dist0, s);
    }
    LG_HIP(h, hipMemsetAsync(c.red.key, 0, sizeof(unsigned long long) * B, s));
    LG_HIP(h, hipMemsetAsync(c.red.any, 0, sizeof(int32_t) * B, s));
    {
        LgFuseArgs a;
        memset(&a, 0, sizeof(a));
        a.approach = planes[LG_MAP_APPROACH]; a.sdf = planes[LG_MAP_SDF]; a.flat = planes[LG_MAP_FLATNESS];
        a.stem = planes[LG_MAP_STEM]; a.dist = planes[LG_MAP_DISTANCE]; a.tip = planes[LG_NUM_MAPS];
        a.safe = safe; a.win = h->win; a.trad = planes[LG_MAP_TRADITIONAL]; a.valid = ps.valid; a.red = c.red;
        a.B = B; a.H = H; a.W = W;
        a.w_approach = ps.P.w_approach; a.w_sdf = ps.P.w_sdf; a.w_flat = ps.P.w_flat; a.w_tip = CP.w_tip;
        a.min_edge_distance = ps.P.min_edge_distance;
        ProfScope pf(h, "col_fuse", s);
        lg_launch_col_fuse(a, s);
    }
    {
        ProfScope pf(h, "col_pick", s);
        lg_launch_col_pick(c.red, c.sums, depth, c.pick, B, H, W, s);
    }
    LgFinishArgs fa = finish_args(h, ps, 1, false);   // the one-point list: nothing to rescore
    fa.cand_n = c.pick.n; fa.cand_xy = c.pick.xy; fa.cand_info = c.pick.info; fa.slot_frames = B;
    {
        ProfScope pf(h, "finish", s);
        lg_launch_finish(fa, s);
    }
    lg_launch_col_rows(c.pick, fa.out, B, s);
    return return_results(h, ps, results, false, "lg_select_grasp_collect", s);
}

}  // namespace

// ============================================================================ the entries
extern "C" {

int lg_tail_lane_plan(int B, int requested, int eligible, int32_t* lanes, int32_t* sb) {
    if (B < 1 || requested < 0 || requested > 4 || !lanes || !sb) return LG_ERR_INVALID;
    int want = requested ? requested : (B >= LG_TAIL_LANES_MIN_B ? LG_TAIL_LANES_AUTO : 1);
    if (!eligible) want = 1;
    want = std::min(want, B);            // a lane never holds fewer than one frame
    *sb = (B + want - 1) / want;
    *lanes = (B + *sb - 1) / *sb;        // (7 frames in 4 lanes: 2 + 2 + 2 + 1; 5 in 4: 2 + 2 + 1, three lanes)
    return LG_OK;
}

int lg_debug_tail_lanes(lg_handle h, int set, int32_t* last) {
    if (!h || set > 4) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (set >= 0) h->tail_lanes_req = set;
    if (last) *last = h->last_tail_lanes;
    return LG_OK;
}

int lg_score_maps(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                  float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid, float* theta_host, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    Plan pl;
    int rc = make_plan(h, pl, depth, mask, B, H, W, pin, out_maps, out_valid);
    if (rc) return rc;
    if (lg_label_aware_check(&pl.P, 0)) return fail(h, LG_ERR_INVALID, "lg_score_maps: label_aware needs the label image (lg_select_grasp_labels, lg_select_grasp_candidates_labels)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure_ws(h, B, H, W, pl.P.top_k))) return rc;
    if ((rc = take_planes(h, pl, false))) return rc;
    // (orientation: lg_orient_kernel beside the distance-transform sweeps, host threads for frames it hands back)
    LgFinalArgs fargs;
    if ((rc = enq_front(h, pl, s, &fargs, nothing_after_prep))) return rc;
    if (theta_host)
        for (int b = 0; b < B; b++) theta_host[b] = h->fp_host[b].theta;
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

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
    const int rc = labels_stage(h, labels, leaf_ids, B, H, W, stream_);
    if (rc) return rc;
    return lg_select_grasp_impl(h, depth, h->mask_ws, labels, B, H, W, pin, out_maps, out_valid, results, nullptr, stream_);
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
    const int rc = labels_stage(h, labels, leaf_ids, B, H, W, stream_);
    if (rc) return rc;
    return lg_select_grasp_impl(h, depth, h->mask_ws, labels, B, H, W, pin, nullptr, nullptr, results, cands, stream_);
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

// ---- the collecting selector and its stages on their own
int lg_collect_params_check(const lg_params* p, const lg_collect_params* cp) {
    int code = LG_OK;
    collect_params_error(p, cp, &code);
    return code;
}

int lg_select_grasp_collect(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* pin,
                            const lg_collect_params* cp, float* const out_maps[LG_NUM_MAPS], float* out_tip, uint8_t* out_safe,
                            uint8_t* out_valid, lg_grasp_result* results, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    return lg_select_grasp_collect_impl(h, depth, mask, B, H, W, pin, cp, out_maps, out_tip, out_safe, out_valid, results, stream_);
}

int lg_erode_ellipse(lg_handle h, const uint8_t* mask, int B, int H, int W, int k, int iterations, uint8_t* out, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!mask || !out || B < 1 || H < 1 || W < 1 || W > 8192 || H > 16384)
        return fail(h, LG_ERR_INVALID, "lg_erode_ellipse: bad pointer or shape (W <= 8192, H <= 16384)");
    lg_collect_params cp;
    lg_default_collect_params(&cp);
    cp.erosion_kernel_size = k; cp.erosion_iterations = iterations;
    int rc = LG_OK;
    if (const char* why = collect_params_error(nullptr, &cp, &rc)) return fail(h, rc, (std::string("lg_erode_ellipse: ") + why).c_str());
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    if ((rc = ensure_ws(h, B, H, W, 20))) return rc;
    if ((rc = col_ensure(h, B, H, W))) return rc;
    reset_last(h);
    const int WW = (W + 63) / 64;
    LG_HIP(h, hipMemsetAsync(h->maxfix, 0, sizeof(uint32_t) * LG_MF * B, s));   // (the bounding boxes accumulate from zero)
    lg_launch_pack_bits(mask, h->bits, B, H, W, WW, s, h->maxfix);
    lg_launch_window(h->maxfix, h->win, B, H, W, 0, s);
    enq_erode(h, B, H, W, WW, k, iterations, out, false, s);
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_tip_penalty(lg_handle h, const uint8_t* safe, int B, int H, int W, const lg_params* pin, const lg_collect_params* cp,
                   float* out, uint8_t* out_tip_area, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!safe || !out || B < 1 || H < 1 || W < 1 || W > 8192 || H > 16384)
        return fail(h, LG_ERR_INVALID, "lg_tip_penalty: bad pointer or shape (W <= 8192, H <= 16384)");
    lg_params P;
    if (pin) P = *pin; else lg_default_params(&P);
    if (P.chamfer_init_dist0 < (int32_t)LG_INIT0)
        return fail(h, LG_ERR_INVALID, "lg_tip_penalty: chamfer_init_dist0 must be in [INT_MAX >> 2, INT_MAX]");
    int rc = LG_OK;
    if (const char* why = collect_params_error(&P, cp, &rc)) return fail(h, rc, (std::string("lg_tip_penalty: ") + why).c_str());
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    {
        ProfScope ps(h, "col_tip", s);
        lg_launch_col_tip(safe, out, B, H, W, (uint32_t)P.chamfer_init_dist0, s);
    }
    if (out_tip_area) LG_HIP(h, hipMemsetAsync(out_tip_area, 0, (size_t)B * H * W, s));   // (no tip area as written)
    LG_HIP(h, hipGetLastError());
    return LG_OK;
}

int lg_argmax_first(lg_handle h, const float* plane, int B, int H, int W, int32_t* xy_host, float* max_host,
                    int32_t* any_positive_host, void* stream_) {
    if (!h) return LG_ERR_INVALID;
    LG_ENTER(h);
    if (!plane || B < 1 || H < 1 || W < 1 || (unsigned long long)H * W > 0xFFFFFFFFull)
        return fail(h, LG_ERR_INVALID, "lg_argmax_first: bad pointer or shape (H * W below 2^32)");
    hipStream_t s = (hipStream_t)stream_;
    LG_HIP(h, hipSetDevice(h->device));
    int rc = col_ensure(h, B, 1, 1);
    if (rc) return rc;
    LgColWs& c = h->col;
    LG_HIP(h, hipMemsetAsync(c.red.key, 0, sizeof(unsigned long long) * B, s));
    LG_HIP(h, hipMemsetAsync(c.red.any, 0, sizeof(int32_t) * B, s));
    {
        ProfScope ps(h, "col_argmax", s);
        lg_launch_col_argmax(plane, c.red, B, H, W, s);
    }
    LG_HIP(h, hipMemcpyAsync(c.key_host, c.red.key, sizeof(unsigned long long) * B, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipMemcpyAsync(c.any_host, c.red.any, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    LG_HIP(h, hipStreamSynchronize(s));
    LG_HIP(h, hipGetLastError());
    for (int b = 0; b < B; b++) {
        float v;
        uint32_t idx;
        lg_argmax_unkey(c.key_host[b], &v, &idx);
        if (xy_host) { xy_host[2 * b] = (int32_t)(idx % (uint32_t)W); xy_host[2 * b + 1] = (int32_t)(idx / (uint32_t)W); }
        if (max_host) max_host[b] = v;
        if (any_positive_host) any_positive_host[b] = c.any_host[b] ? 1 : 0;
    }
    return LG_OK;
}

}  // extern "C"
