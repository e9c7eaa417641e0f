// Distance transform (lg_dt.hip): the chamfer-5 norm and what follows from it in closed form (the border search, the sweep
// window), launchers of its kernels and the choice between the forms of the sweep-free row search.
#pragma once
#include "lg_internal.h"

// lg_window_kernel, search_mode 2: a batch's d_in comes from the row search while sum over its frames of area^1.5 <= this *
// (rows of its tallest bounding box)
#ifndef LG_SEARCH_BUDGET
#define LG_SEARCH_BUDGET 2.0e7f
#endif

__host__ __device__ inline uint32_t lg_norm5(int dx, int dy) {   // closed-form norm of the (1, 1.4, 2.1969) chamfer mask
    const uint32_t a = (uint32_t)(dx > dy ? dx : dy), b = (uint32_t)(dx > dy ? dy : dx);
    return 2u * b <= a ? (a - 2u * b) * LG_A5 + b * LG_C5 : (a - b) * LG_C5 + (2u * b - a) * LG_B5;
}
// OpenCV's transform keeps chamfer_init_dist0 in the border cells around the image, so a pixel's value is
//     min(distance to the nearest source, init0 + a * (steps to the nearest border cell)).
// The second term can only win in a frame where a distance can reach init0 (INT_MAX >> 2 is 8192 px: frames taller than 8192 rows,
// or 8192 columns wide and a few rows high).  Such a frame is swept whole -- no window, no closed-form border maximum, no row
// search -- and lg_dt5_kernel applies the border term to every pixel; every other frame cannot tell the difference.
__host__ __device__ inline bool lg_dt_far(int H, int W, uint32_t init0) { return lg_norm5(W - 1, H - 1) >= init0; }

// ---- max d_out along one frame border line (lg_dout_border_kernel; host export lg_border_line_max)
// prof[i], i in [0, n): distance from the border line of the nearest leaf pixel in line position lo + i (-1: none).  A candidate
// p on the line has d_out(p) = min over the entries i with prof[i] >= 0 of lg_norm5(|p - (lo + i)|, prof[i]); the line's maximum
// lies among p in {lo .. lo + n - 1, 0, len - 1} (see the kernel).  lg_norm5 is monotone in both arguments, which gives an exact
// pruned search: the two ends are evaluated in full (lg_border_end_part) and seed `best`; a span candidate visits the entries
// outwards from its own position, i = c - k and c + k for k = 0, 1, ..., and stops
//   (a) once its running minimum dmin <= best: dmin only falls, the candidate cannot raise the maximum;
//   (b) once lg_norm5(k, m) >= dmin, m = the smallest entry >= 0: no entry at distance >= k can lower dmin;
//   (c) when both directions have left the profile.
// (b) and (c) leave dmin exact, (a) drops only candidates bounded by a value already attained: the maximum keeps its bits.
__host__ __device__ inline uint32_t lg_border_cand_min(const int32_t* prof, int n, int c, int m, uint32_t best) {
    uint32_t dmin = 0xFFFFFFFFu;
    for (int k = 0; k < n; k++) {
        const int il = c - k, ir = c + k;
        if (il < 0 && ir >= n) break;                                   // (c)
        if (lg_norm5(k, m) >= dmin) break;                              // (b)
        if (il >= 0) { const int d = prof[il]; if (d >= 0) { const uint32_t v = lg_norm5(k, d); dmin = v < dmin ? v : dmin; } }
        if (ir < n && k) { const int d = prof[ir]; if (d >= 0) { const uint32_t v = lg_norm5(k, d); dmin = v < dmin ? v : dmin; } }
        if (dmin <= best) break;                                        // (a)
    }
    return dmin;
}
// entries t, t + nt, ... of the profile against line position p: their minimum (0xFFFFFFFF: none of them holds a leaf pixel)
__host__ __device__ inline uint32_t lg_border_end_part(const int32_t* prof, int n, int lo, int p, int t, int nt) {
    uint32_t dmin = 0xFFFFFFFFu;
    for (int i = t; i < n; i += nt) {
        const int d = prof[i], dx = p - (lo + i);
        if (d >= 0) { const uint32_t v = lg_norm5(dx < 0 ? -dx : dx, d); dmin = v < dmin ? v : dmin; }
    }
    return dmin;
}
// The whole search by one thread, as the kernel's 256 threads compose it (ends, then the span against the running maximum).
// *out = 0xFFFFFFFF when no entry holds a leaf pixel (every candidate's minimum is over nothing).
__host__ __device__ inline void lg_border_search(const int32_t* prof, int n, int lo, int len, uint32_t* out) {
    int m = 0x7fffffff;
    for (int i = 0; i < n; i++) if (prof[i] >= 0 && prof[i] < m) m = prof[i];
    if (m == 0x7fffffff) { *out = 0xFFFFFFFFu; return; }
    const uint32_t e0 = lg_border_end_part(prof, n, lo, 0, 0, 1), e1 = lg_border_end_part(prof, n, lo, len - 1, 0, 1);
    uint32_t best = e0 > e1 ? e0 : e1;
    for (int c = 0; c < n; c++) {
        const uint32_t d = lg_border_cand_min(prof, n, c, m, best);
        best = d > best ? d : best;
    }
    *out = best;
}

// A frame's LgWin from the five words the bit-row pass accumulated (box = &maxfix[frame * LG_MF + LG_BOX_X0], see LG_MF).  wc,
// nw_max: lg_dt_geometry(W).  search_in is the frame's own eligibility (search_mode != 0, a non-empty mask with at least one
// zero pixel); lg_window_kernel clears it for the whole batch when the sweeps win (search_mode 2).  lg_window_kernel and the
// host export lg_window_from_box run this code.
__host__ __device__ inline LgWin lg_win_from_box(const uint32_t box[5], int H, int W, int wc, int nw_max, int search_mode) {
    LgWin w;
    w.area = (int)box[LG_BOX_AREA - LG_BOX_X0];
    w.search_in = 0;
    if (w.area == 0) {   // empty mask: no window (d_out has no source: the closed form of the whole frame applies)
        w.bx0 = 0; w.bx1 = -1; w.by0 = 0; w.by1 = -1;
        w.wx0 = 0; w.nw = nw_max; w.wy0 = 0; w.wy1 = H;
        w.skip_out = 0;
    } else {
        w.bx0 = W - 1 - (int)box[LG_BOX_X0 - LG_BOX_X0]; w.bx1 = (int)box[LG_BOX_X1 - LG_BOX_X0];
        w.by0 = H - 1 - (int)box[LG_BOX_Y0 - LG_BOX_X0]; w.by1 = (int)box[LG_BOX_Y1 - LG_BOX_X0];
        // d_in by the row search (lg_dtsearch_kernel) needs a zero pixel in the image (a frame without one has OpenCV's
        // border-initialised result, which only the sweeps produce)
        w.search_in = (search_mode != 0 && (long long)w.area < (long long)H * W) ? 1 : 0;
        w.wx0 = (w.bx0 / LG_TW) * LG_TW;
        w.nw = (w.bx1 + 1 - w.wx0 + wc - 1) / wc;
        w.wy0 = (w.by0 / LG_TH) * LG_TH;
        const int wy1 = ((w.by1 + 1 + LG_TH - 1) / LG_TH) * LG_TH;
        w.wy1 = wy1 < H ? wy1 : H;
        // Only max d_out is consumed (grasp_point_selector.py:531-533).  Inside the window d_out(p) <= N(p - q) for any leaf
        // pixel q, and both lie in the window: <= N(window width - 1, window height - 1).  At a frame corner every leaf pixel is
        // at least the corner's gap to the bounding box away in x and in y: d_out(corner) >= N(gap_x, gap_y) (N is monotone in
        // both).  When the best corner bound exceeds the window bound, the maximum is the frame-border maximum that
        // lg_dout_border_kernel computes exactly, and the two d_out sweeps of this frame have nothing to add: they are skipped
        // (the usual case: a leaf is a few hundred pixels across, the frame's far corner a thousand away).
        const int wend = w.wx0 + w.nw * wc;
        const int ww = (wend < W ? wend : W) - w.wx0, wh = w.wy1 - w.wy0;
        const uint32_t ub_in = lg_norm5(ww - 1, wh - 1);
        const int gx = w.bx0 > W - 1 - w.bx1 ? w.bx0 : W - 1 - w.bx1, gy = w.by0 > H - 1 - w.by1 ? w.by0 : H - 1 - w.by1;
        // (strictly larger: the corner that achieves it then lies outside the window, on a border line lg_dout_border_kernel walks)
        w.skip_out = lg_norm5(gx, gy) > ub_in ? 1 : 0;
    }
    w.pad_[0] = 0;
    return w;
}

// columns per sweep wave / waves per sweep workgroup for width W (0 if unsupported)
int lg_dt_geometry(int W, int* waves);
// search_mode: 0 = d_in by the two sweeps for every frame, 1 = by the row search wherever it applies (a non-empty mask with
// at least one zero pixel), 2 = the row search when the batch's estimated search work stays below the sweeps' latency
// mf: what lg_launch_pack_bits / lg_launch_pack_labels accumulated on the same stream
// init0: lg_params.chamfer_init_dist0 of a call whose windows the distance transforms will use (lg_dt_far); the orientation-only
// callers leave it out
void lg_launch_window(const uint32_t* mf, LgWin* win, int B, int H, int W, int search_mode, hipStream_t s, uint32_t init0 = 0xFFFFFFFFu);
int lg_launch_dt(bool bwd, const uint8_t* mask, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                 int H, int W, uint32_t init0, hipStream_t s);   // init0: lg_params.chamfer_init_dist0 (frames without a zero pixel)
// max d_out outside the sweep windows (closed-form chamfer norm on the frame border) -> atomicMax into maxfix[b][1]
void lg_launch_dout_border(const unsigned long long* bits, const LgWin* win, uint32_t* maxfix, int B, int H, int W, int WW,
                           hipStream_t s);

// ---- d_in without the row-sequential sweeps (frames with LgWin::search_in): horizontal run distances of the bounding-box rows
// into `tmp` (the d_in half of the sweep workspace, as uint16), then one form of the search over rows, which writes distance_map
// inside the window and the maximum into maxfix[b][0].  The numbering is LG_DT_SEARCH_ALGO's and lg_debug_dt_search_form's
// (2, 3 and 4 were the two-level search with recorded minimising rows: DESIGN.md).
enum {
    LG_DT_FORM_ROWS = 1,    // every row by the bounded search over rows: lg_launch_dt_rows
    LG_DT_FORM_BANDS = 5,   // pairs of adjacent seed rows by that search, the rows between two pairs by the chamfer stencil run
                            // down and up in registers: lg_launch_dt_seeds, then lg_launch_dt_bands.  H, W >= 16
    LG_DT_FORM_SWEEP = 6,   // the whole bounding box by that stencil, one workgroup per frame: lg_launch_dt_sweep.  H >= 16,
                            // 16 <= W <= 2048
};
// The form a batch of n frames of H x W takes; forced = LG_DT_SEARCH_ALGO (0: by size).  One level up to 64 frames of 1080p (one
// launch, the device is not full: 32 of 1080p 0.14 vs 0.18 ms).  Above, the register sweep when a bounding box's span fits 64
// lanes x 32 columns, W <= 2048: 256 of 1080p 0.229 ms against 0.235 + 0.140 for seed pairs + bands, and one workgroup per CU
// instead of 32 k workgroups beside the side chain (profiles/NOTES_dt_sweep.md); 4K keeps seed pairs + bands
// (profiles/NOTES_dt_bands.md).  The seed rows of form 5 share the run distances' workspace and need the room of sixteen rows
// and columns, form 6 likewise: lower or narrower frames take form 1 whatever is asked for.
inline int lg_dt_form(int forced, int n, int H, int W) {
    const bool bands_ok = H >= 16 && W >= 16, sweep_ok = bands_ok && W <= 2048;
    const int big = sweep_ok ? LG_DT_FORM_SWEEP : bands_ok ? LG_DT_FORM_BANDS : LG_DT_FORM_ROWS;
    switch (forced) {
        case LG_DT_FORM_ROWS: return LG_DT_FORM_ROWS;
        case LG_DT_FORM_BANDS: return bands_ok ? LG_DT_FORM_BANDS : LG_DT_FORM_ROWS;
        case LG_DT_FORM_SWEEP: return big;
        default: return (long long)n * H * W <= 64ll * 1080 * 1920 ? LG_DT_FORM_ROWS : big;
    }
}
void lg_launch_hrun(const unsigned long long* bits, uint32_t* tmp, const LgWin* win, int B, int H, int W, int WW, hipStream_t s);
void lg_launch_dt_rows(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                       int H, int W, int WW, hipStream_t s);
// band_p = 12 | 16 | 24 | 32 (else 16): rows from one seed pair to the next; band_e = 2 | 4: columns per lane of the band kernel
void lg_launch_dt_seeds(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, hipStream_t s);
void lg_launch_dt_bands(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, int band_e, hipStream_t s);
void lg_launch_dt_sweep(uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B, int H, int W, hipStream_t s);
