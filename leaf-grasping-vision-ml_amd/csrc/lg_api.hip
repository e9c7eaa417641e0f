// C-ABI of liblgrasp.so (see include/leafgrasp.h), all but grasp selection (lg_select.hip): the handle's life (lg_ctx.h), errors,
// per-kernel event timing, the debug and host-helper entries, the single-stage entries.  No exceptions cross the boundary.
#include <string.h>

#include <algorithm>

#include "lg_ctx.h"
#include "lg_dt.h"
#include "lg_eval.h"

#define LG_VERSION_STR "leafgrasp-gfx950 0.4"

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
    col_free(h);
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

void lg_default_collect_params(lg_collect_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->erosion_kernel_size = 21; p->erosion_iterations = 2;   // grasp_point_selector_bkp.py:30-31
    p->tip_se = 15;                                           // :397
    p->tip_aware = 0;
    p->w_tip = 0.1f;                                          // :102
}

// cv2.erode(bits, ellipse k, iterations) on the host, the device's per-word code (lg_collect.h): complemented rows, one dilation
// per iteration on the words of the mask's bounding box, complemented back
int lg_erode_words_host(const uint64_t* bits, int H, int W, int WW, int k, int iterations, uint64_t* out) {
    if (!bits || !out || H < 1 || W < 1 || WW != (W + 63) / 64) return LG_ERR_INVALID;
    if (k < 1 || k > 63 || !(k & 1) || iterations < 0 || iterations > 8) return LG_ERR_UNSUPPORTED;
    LgSeSpans se;
    lg_make_se_spans(k, &se);
    LgStemPlan sp;
    lg_make_stem_plan(se, &sp);
    std::vector<unsigned long long> a((size_t)H * WW), b((size_t)H * WW);
    int bx0 = W, bx1 = -1, by0 = H, by1 = -1;
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) {
            const unsigned long long fm = lg_frame_word_mask(W, WW, w), v = (unsigned long long)bits[(size_t)y * WW + w] & fm;
            a[(size_t)y * WW + w] = ~v & fm;
            if (!v) continue;
            bx0 = std::min(bx0, 64 * w + __builtin_ctzll(v));
            bx1 = std::max(bx1, 64 * w + 63 - __builtin_clzll(v));
            by0 = std::min(by0, y);
            by1 = y;
        }
    for (int i = 0; i < iterations; i++) {
        for (int y = 0; y < H; y++)
            for (int w = 0; w < WW; w++) b[(size_t)y * WW + w] = lg_erode_step_word(a.data(), H, W, WW, y, w, bx0, bx1, by0, by1, se, sp);
        a.swap(b);
    }
    for (int y = 0; y < H; y++)
        for (int w = 0; w < WW; w++) out[(size_t)y * WW + w] = ~a[(size_t)y * WW + w] & lg_frame_word_mask(W, WW, w);
    return LG_OK;
}

int lg_tip_fix_host(int H, int W, int32_t chamfer_init_dist0, uint32_t* out, uint32_t* max_fix) {
    if (!out || H < 1 || W < 1 || W > 8192 || H > 16384 || chamfer_init_dist0 < (int32_t)LG_INIT0) return LG_ERR_INVALID;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) out[(size_t)y * W + x] = lg_tip_fix(x, y, H, W, (uint32_t)chamfer_init_dist0);
    if (max_fix) *max_fix = lg_tip_fix_max(H, W, (uint32_t)chamfer_init_dist0);
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

// ============================================================================ ML-only grasp selection (lg_mlsel.h): host helpers
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

}  // extern "C"
