// The collecting selector (lg_collect.hip; include/leafgrasp.h lg_select_grasp_collect): the variant of
// select_grasp_point that feeds the data collector (scripts/utils/grasp_point_selector_bkp.py:73-169) -- ellipse erosion on bit
// rows, the tip-penalty plane, the variant's fusion and validity, and a batched first-maximum arg-max with the centroid of the
// original mask behind it.  What the device and the host exports share is here, next to the launchers.
#pragma once
#include "lg_internal.h"   // (ends with the stage headers: the bit-row code below builds on lg_bits.h, so this one is not among them)

// ---- ellipse erosion on bit rows: cv2.erode(mask, ellipse k, iterations = n) (bkp:79-82)
// The ellipse is symmetric under a half turn, so one erosion is the complement of the dilation of the complement, the complement
// taken as 0 outside the frame (the border does not erode).  The rows are therefore kept COMPLEMENTED from the first pass to the
// last: c_0 = ~mask inside the frame, c_{i + 1} = cv2.dilate(c_i, ellipse) (lg_frame_dilate_word: the stem chains with the whole
// frame as their source, restricted to the frame), safe = ~c_n inside the frame.  An erosion never sets a pixel, so outside the
// words of the mask's bounding box every c_i is all ones: those words are written without arithmetic.
__host__ __device__ inline unsigned long long lg_frame_word_mask(int W, int WW, int w) {   // the pixels of word w that lie in the frame
    return (w == WW - 1 && (W & 63)) ? (~0ull >> (64 - (W & 63))) : ~0ull;
}
// words [w0, w1] x rows [y0, y1] of the bounding box (bx1 < bx0: empty mask, no word)
__host__ __device__ inline bool lg_erode_word_in_box(int bx0, int bx1, int by0, int by1, int y, int w) {
    return bx1 >= bx0 && by1 >= by0 && y >= by0 && y <= by1 && w >= (bx0 >> 6) && w <= (bx1 >> 6);
}
// one word of c_{i + 1} from the rows of c_i
__host__ __device__ inline unsigned long long lg_erode_step_word(const unsigned long long* comp, int H, int W, int WW, int y, int w,
                                                                 int bx0, int bx1, int by0, int by1, const LgSeSpans& se,
                                                                 const LgStemPlan& pl) {
    if (!lg_erode_word_in_box(bx0, bx1, by0, by1, y, w)) return lg_frame_word_mask(W, WW, w);
    return lg_frame_dilate_word(comp, H, W, WW, y, w, se, pl);
}

// ---- the tip penalty as written (bkp:395-408): `(~tip_area).astype(np.uint8)` of a 0 / 1 image has no zero pixel, so the 5 x 5
// transform is the degenerate one of DESIGN 2 quirk 1: border cells of init0 around the frame, one straight step of 1.0 per pixel
// towards the nearest frame line.  16.16 integers; the whole-frame maximum sits at the frame's middle.
__host__ __device__ inline uint32_t lg_tip_fix(int x, int y, int H, int W, uint32_t init0) {
    int m = x + 1 < y + 1 ? x + 1 : y + 1;
    m = W - x < m ? W - x : m;
    m = H - y < m ? H - y : m;
    return init0 + LG_A5 * (uint32_t)m;
}
__host__ __device__ inline uint32_t lg_tip_fix_max(int H, int W, uint32_t init0) {
    const int m = (W + 1) / 2 < (H + 1) / 2 ? (W + 1) / 2 : (H + 1) / 2;
    return init0 + LG_A5 * (uint32_t)m;
}
// penalty = 1 - d / (max(d) + 1e-6) on a pixel of `safe`, by the float32 rules of the isolation plane (lg_iso_value)
__host__ __device__ inline float lg_tip_value(uint32_t d_fix, uint32_t max_fix) {
#pragma clang fp contract(off)
    const float k = 1.0f / 65536.0f;
    return 1.0f - ((float)d_fix * k) / ((float)max_fix * k + 1e-6f);
}

// ---- first maximum in row-major order, a NaN counting as the maximum (np.argmax): one 64-bit key per pixel, larger = better --
// the float's bits made monotonic (every NaN the largest, -0.0 = +0.0) above the complement of the flat index
__host__ __device__ inline unsigned long long lg_argmax_key(float v, uint32_t idx) {
    uint32_t u;
    if (v != v) {
        u = 0xFFFFFFFFu;
    } else {
        if (v == 0.0f) v = 0.0f;
        union { float f; uint32_t i; } c;
        c.f = v;
        u = (c.i >> 31) ? ~c.i : (c.i | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
__host__ __device__ inline void lg_argmax_unkey(unsigned long long key, float* v, uint32_t* idx) {
    const uint32_t u = (uint32_t)(key >> 32);
    union { float f; uint32_t i; } c;
    c.i = (u == 0xFFFFFFFFu) ? 0x7FC00000u : (u >> 31) ? (u & 0x7FFFFFFFu) : ~u;
    *v = c.f;
    *idx = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
}

// ---- per-frame words of a collecting call
#define LG_COL_SUMS 4   // [0] sum x, [1] sum y, [2] set pixels of the ORIGINAL mask (64-bit sums), [3] unused
struct LgColReduce {
    unsigned long long* key;   // [B] atomicMax of lg_argmax_key over the frame, zeroed by the caller (0: below every key)
    int32_t* any;              // [B] != 0: some value > 0
};
// what the pick leaves for lg_finish_kernel (a one-point list) and for the rows behind it
struct LgColPick {
    int32_t* n;       // [B] 1: a point (arg-max or centroid), 0: empty original mask
    int32_t* xy;      // [B][2]
    float* info;      // [B][2] np.max(trad), depth at the point
    int32_t* meta;    // [B][2] n_candidates (1 arg-max, 0 centroid), best_score bits
};

// the handle's workspace of the collecting entries (lg_select.hip owns it), grown on demand
struct LgColWs {
    size_t cap_words = 0, cap_px = 0;
    int cap_B = 0;
    unsigned long long* comp[2] = {nullptr, nullptr};   // [B][H][WW] complemented rows, ping and pong
    uint8_t* safe = nullptr;                            // [B][H][W], when the caller does not take it back
    float* planes[LG_NUM_MAPS + 1] = {nullptr};         // [B][H][W] each, on first use: the planes the caller leaves out; [8] tip
    unsigned long long* sums = nullptr;                 // [B][LG_COL_SUMS]
    LgColReduce red = {nullptr, nullptr};
    LgColPick pick = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long* key_host = nullptr;             // pinned [B], lg_argmax_first
    int32_t* any_host = nullptr;                        // pinned [B]
};

struct LgFuseArgs {
    const float *approach, *sdf, *flat, *stem, *dist, *tip;   // [B][H][W]; approach, sdf, stem, dist, tip computed on `safe`
    const uint8_t* safe;                                       // [B][H][W] 0 / 1
    const LgWin* win;                                          // [B] bounding boxes of `safe`
    float* trad;                                               // out [B][H][W]
    uint8_t* valid;                                            // out [B][H][W]
    LgColReduce red;
    int B, H, W;
    float w_approach, w_sdf, w_flat, w_tip, min_edge_distance;
};

// ---- launchers (lg_collect.hip), every launch over the frames [0, B) of its pointers
// comp[b] = ~bits[b] inside the frame; sums (null: not wanted; zeroed by the caller): the centroid numerators of bits[b]
void lg_launch_col_complement(const unsigned long long* bits, unsigned long long* comp, unsigned long long* sums, int B, int H, int W,
                              int WW, hipStream_t s);
// dst[b] = cv2.dilate(src[b], ellipse k) on the words of win[b]'s bounding box, all ones elsewhere
void lg_launch_col_erode_step(const unsigned long long* src, unsigned long long* dst, const LgWin* win, int B, int H, int W, int WW, int k,
                              hipStream_t s);
// safe[b] = ~comp[b] inside the frame as 0 / 1 bytes
void lg_launch_col_unpack(const unsigned long long* comp, uint8_t* safe, int B, int H, int W, int WW, hipStream_t s);
// out[b] = the tip penalty as written on the pixels of safe[b], 0 elsewhere
void lg_launch_col_tip(const uint8_t* safe, float* out, int B, int H, int W, uint32_t init0, hipStream_t s);
void lg_launch_col_fuse(const LgFuseArgs& a, hipStream_t s);
// the reduction alone on a handed plane
void lg_launch_col_argmax(const float* plane, const LgColReduce& red, int B, int H, int W, hipStream_t s);
// arg-max or centroid of every frame -> the one-point list
void lg_launch_col_pick(const LgColReduce& red, const unsigned long long* sums, const float* depth, const LgColPick& pick, int B, int H,
                        int W, hipStream_t s);
// behind lg_finish_kernel: n_candidates, ml_used and best_score of the rows
void lg_launch_col_rows(const LgColPick& pick, lg_grasp_result* res, int B, hipStream_t s);
