// Internal declarations shared by the HIP translation units of liblgrasp.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/leafgrasp.h"

// ---- chamfer constants: 16.16 fixed point of OpenCV's DIST_L2 masks ("Distance transform")
#define LG_A5 65536u        // 1.0
#define LG_B5 91750u        // 1.4
#define LG_C5 143976u       // 2.1969
#define LG_A3 62587u        // 0.955
#define LG_B3 89738u        // 1.3693
#define LG_INIT0 0x1FFFFFFFu  // INT_MAX >> 2 : OpenCV's border initialiser, the default of lg_params.chamfer_init_dist0
#define LG_INF 0x3FFFFFFFu    // "no path yet" inside the DT sweeps (never wins against a real distance)
#define LG_NOSRC 0x20000000u  // 8192 px: with chamfer_init_dist0 up to here OpenCV's border cells hide every distance near LG_INF (make_plan)
#define LG_HCAP 16383u        // run distance of a row without any zero pixel in the image (row search; W <= 8192)
// lg_window_kernel, search_mode 2: a batch's d_in comes from the row search while sum over its frames of area^1.5 <= this *
// (rows of its tallest bounding box)
#ifndef LG_SEARCH_BUDGET
#define LG_SEARCH_BUDGET 2.0e7f
#endif
// Words per frame of the `maxfix` array, zeroed by one memset in front of the bit-row pass:
//   [0], [1]  max fixed-point d_in / d_out (atomicMax of the distance transform)
//   [2 .. 6]  the mask's bounding box and area as the bit-row pass accumulates them (LG_BOX_*): every word is a maximum or a
//             sum over the set bits, so all start from 0 -- the two minima are held as W - 1 - x0 and H - 1 - y0; a frame
//             whose area stayed 0 has no set bit, whatever the other four say
#define LG_MF 8
#define LG_BOX_X0 2   // max of W - 1 - x
#define LG_BOX_X1 3   // max of x
#define LG_BOX_Y0 4   // max of H - 1 - y
#define LG_BOX_Y1 5   // max of y
#define LG_BOX_AREA 6 // number of set bits


#define LG_MAX_GAUSS 15   // largest smoothing kernel lg_smooth_depth takes (the fused plane kernel: 1, 3, 5, 7)
struct LgGaussTaps { float k[LG_MAX_GAUSS]; };   // 1-D factor of ImageProcessor's Gaussian (by value in the kernel arguments)

// ---- final-kernel tile
#define LG_TW 64
#ifndef LG_TH
#define LG_TH 16   // measured at 1080p B=128: 16 -> 1.78 ms (0.69 of HBM peak), 32 -> 1.86 ms, 64 -> 2.11 ms (round 1); round 2, whole library
                   // built with -DLG_TH=32: planes 2.60-2.71 vs 2.66-2.74 ms per 256 frames, top-k 0.33 vs 0.27 ms, dense launch the same
#endif

// Window of the distance-transform sweeps (per frame, written by lg_window_kernel).  The binary leaf mask covers a few
// per cent of a frame, so the sweeps run on the tile-aligned window around its bounding box only:
//   d_in  (distance to the nearest zero pixel): every pixel outside the window is itself a zero pixel -> exactly 0, and
//         enters the window as a 0-valued halo: the windowed two-pass recurrence is the full-frame one, bit for bit.
//   d_out (distance to the leaf; only max d_out is consumed): the two-pass 5x5 chamfer transform equals
//         min over sources of the chamfer NORM (weights satisfy 2a <= c <= a+b, 3b <= 2c), shortest paths stay inside the
//         bounding rectangle of their end points, so the window computed as a stand-alone image is exact inside; outside
//         the window the distance grows monotonically towards the frame border, where lg_dout_border_kernel evaluates
//         the norm in closed form against the leaf's row / column profiles.
// Columns [wx0, wx0 + nw * 64 * E) (clipped to W), rows [wy0, wy1): wx0 % 64 == 0, wy0 % LG_TH == 0, so every tile of
// the fused score-plane kernel is either inside (reads distance_map) or outside (writes zeros to it).
struct LgWin {
    int wx0, nw, wy0, wy1;   // window: first column, active waves (64*E columns each), row range
    int bx0, bx1, by0, by1;  // bounding box of the mask (bx1 < bx0: empty mask -> window = whole frame)
    int skip_out;            // 1: max d_out cannot lie inside the window (see lg_win_from_box): the d_out sweeps of this frame are skipped
    int search_in;           // 1: d_in of this frame comes from the row search (lg_hrun_kernel + lg_dtsearch_kernel), its d_in sweeps are skipped
    int area;                // set bits of the mask
    int pad_[1];
};

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

// Near tiles of a frame: the tiles of the fused score-plane kernel (LG_TW x LG_TH, stencil reach `halo` = Gaussian radius + 1)
// whose bit-row test can meet the mask's bounding box [bx0, bx1] x [by0, by1].  The test reads columns tx0-8 .. tx0+LG_TW+7 and
// rows ty0-halo .. ty0+LG_TH-1+halo reflected at the frame border -- at the bottom that reaches up to LG_TH+halo rows above ty0
// (a last tile row of one pixel), at the top it stays inside the tile -- so tile (tx, ty), tx0 = tx * LG_TW, ty0 = ty * LG_TH, is
// near when
//     bx1 >= bx0  &&  bx0 <= tx0 + LG_TW + 7  &&  bx1 >= tx0 - 8  &&  by0 <= ty0 + LG_TH - 1 + halo  &&  by1 >= ty0 - LG_TH - halo.
// Each inequality bounds tx or ty alone: the near tiles are the rectangle [*tx_lo, *tx_hi] x [*ty_lo, *ty_hi] of the frame's
// tile grid.  Returns their number; 0 (an empty box, or one that no tile of the grid reaches) with the rectangle (0, -1, 0, -1).
// Every other tile is constant whatever the mask: key and state byte depend on the tile index alone.  lg_final_kernel, the
// enumeration (lg_near_tiles_kernel) and the host export lg_near_tile_rect run this code.
__host__ __device__ inline int lg_near_tiles(int bx0, int bx1, int by0, int by1, int H, int W, int halo, int* tx_lo, int* tx_hi,
                                             int* ty_lo, int* ty_hi) {
    const int tiles_x = (W + LG_TW - 1) / LG_TW, tiles_y = (H + LG_TH - 1) / LG_TH;
    const int xa = bx0 - (LG_TW + 7), xb = bx1 + 8;                     // xa <= tx0 <= xb
    const int ya = by0 - (LG_TH - 1 + halo), yb = by1 + LG_TH + halo;   // ya <= ty0 <= yb
    const int x_lo = xa > 0 ? (xa + LG_TW - 1) / LG_TW : 0, y_lo = ya > 0 ? (ya + LG_TH - 1) / LG_TH : 0;
    const int x_hi = xb < 0 ? -1 : (xb / LG_TW < tiles_x ? xb / LG_TW : tiles_x - 1);
    const int y_hi = yb < 0 ? -1 : (yb / LG_TH < tiles_y ? yb / LG_TH : tiles_y - 1);
    if (bx1 < bx0 || x_lo > x_hi || y_lo > y_hi) {
        *tx_lo = 0; *tx_hi = -1; *ty_lo = 0; *ty_hi = -1;
        return 0;
    }
    *tx_lo = x_lo; *tx_hi = x_hi; *ty_lo = y_lo; *ty_hi = y_hi;
    return (x_hi - x_lo + 1) * (y_hi - y_lo + 1);
}
__host__ __device__ inline int lg_near_tiles(const LgWin& w, int H, int W, int halo, int* tx_lo, int* tx_hi, int* ty_lo, int* ty_hi) {
    return lg_near_tiles(w.bx0, w.bx1, w.by0, w.by1, H, W, halo, tx_lo, tx_hi, ty_lo, ty_hi);
}

// The plane kernel's wave-level shortcut, as the deferred gather has to evaluate it for one pixel: a wave of lg_final_kernel
// holds four rows of a tile, y & ~3 .. (y & ~3) + 3 (LG_TH % 4 == 0, 16 lanes of 4 pixels per row), over the tile's 64 columns
// = word w = x >> 6 of the bit rows.  When none of those pixels lies on the mask the wave stores +0.0 in every "* mask" plane;
// otherwise a pixel off the mask stores (expression) * 0, which is -0.0 where the expression is negative.  bits: the frame's
// bit rows [H][WW] (bits past W are 0).  lg_gather_kernel and the host export lg_wave_rows_on_mask run this code.
__host__ __device__ inline bool lg_wave_on_mask(const unsigned long long* bits, int H, int WW, int y, int w) {
    const int y4 = y & ~3;
    unsigned long long any = 0;
    for (int r = 0; r < 4; r++)
        if (y4 + r < H) any |= bits[(size_t)(y4 + r) * WW + w];
    return any != 0;
}

struct LgFrameParams {  // per frame: leaf orientation, written by lg_orient_kernel (or by the host analysis for frames it hands back)
    float sin_t, cos_t;
    int has_angle;
    float theta;
};

struct LgSeSpans {  // run-length form of an elliptical structuring element (one span per SE row)
    int n;          // rows
    int anchor;     // k/2
    signed char lo[64];  // first set column - anchor (inclusive); lo > hi => empty row
    signed char hi[64];  // last set column - anchor (inclusive)
};

// ---- stem penalty on the bit rows: stem = dilate(mask & bottom region, ellipse k) & mask (grasp_point_selector.py:688-701)
// dilate(x, y) = OR over the SE rows i and dx in [lo_i, hi_i] of src(x + dx, y + i - anchor) (cv2.dilate, anchor k / 2); src is
// the mask on the rows [bottom_start, H) and zero elsewhere.  One output word = 64 pixels of a row, computed on the 192-bit
// segment of the source rows around it (LgU192); the reach of an ellipse of at most 64 stays below 64 bits.
// lg_stem_bits_kernel / lg_stem_chain_kernel and the host export lg_stem_words_host run this code.
struct LgU192 {
    unsigned long long w0, w1, w2;  // bit p of the segment: w0 = bits 0..63 (word w - 1), w1 = word w, w2 = word w + 1
};
__host__ __device__ inline LgU192 lg_shr192(LgU192 r, int s) {  // out(p) = r(p + s), 0 < s < 64
    LgU192 o;
    o.w0 = (r.w0 >> s) | (r.w1 << (64 - s));
    o.w1 = (r.w1 >> s) | (r.w2 << (64 - s));
    o.w2 = (r.w2 >> s);
    return o;
}
__host__ __device__ inline LgU192 lg_shl192(LgU192 r, int s) {  // out(p) = r(p - s), 0 < s < 64
    LgU192 o;
    o.w2 = (r.w2 << s) | (r.w1 >> (64 - s));
    o.w1 = (r.w1 << s) | (r.w0 >> (64 - s));
    o.w0 = (r.w0 << s);
    return o;
}
__host__ __device__ inline LgU192 lg_or192(LgU192 a, LgU192 b) {
    LgU192 o = {a.w0 | b.w0, a.w1 | b.w1, a.w2 | b.w2};
    return o;
}
// the segment of source row yy around word w: zero outside the bottom region
__host__ __device__ inline LgU192 lg_stem_row192(const unsigned long long* fb, int H, int WW, int bottom_start, int yy, int w) {
    LgU192 r = {0ull, 0ull, 0ull};
    if (yy >= bottom_start && yy < H) {
        const unsigned long long* row = fb + (size_t)yy * WW;
        r.w0 = (w > 0) ? row[w - 1] : 0ull;
        r.w1 = row[w];
        r.w2 = (w + 1 < WW) ? row[w + 1] : 0ull;
    }
    return r;
}
// One output word by the per-row definition: every SE row's segment is dilated by its own span from scratch (doubling).
__host__ __device__ inline unsigned long long lg_stem_word_rows(const unsigned long long* fb, int H, int WW, int bottom_start,
                                                                int y, int w, const LgSeSpans& se) {
    unsigned long long acc = 0;
    for (int i = 0; i < se.n; i++) {
        const int lo = se.lo[i], hi = se.hi[i];
        if (lo > hi) continue;
        const LgU192 r = lg_stem_row192(fb, H, WW, bottom_start, y + i - se.anchor, w);
        if (!(r.w0 | r.w1 | r.w2)) continue;
        // T bit p = OR_{j=0..n} R[p+j]
        const int n = hi - lo;
        LgU192 t = r;
        int covered = 1;  // t covers shifts [0, covered-1]
        while (covered * 2 <= n + 1) {
            t = lg_or192(t, lg_shr192(t, covered));
            covered *= 2;
        }
        if (covered < n + 1) t = lg_or192(t, lg_shr192(t, n + 1 - covered));
        // out bit b = T bit (64 + b + lo)
        unsigned long long o;
        if (lo > 0) o = (t.w1 >> lo) | (t.w2 << (64 - lo));
        else if (lo == 0) o = t.w1;
        else o = (t.w0 >> (64 + lo)) | (t.w1 << -lo);
        acc |= o;
    }
    return acc;
}

// The same word by two chains of nested spans.  The spans of an ellipse are nested from both end rows towards its widest row
// i0; dilation by an interval distributes over OR, and dilations by intervals compose by adding their ends.  So for the rows
// i0, i0 - 1, ..., 0 (and likewise i0, i0 + 1, ..., n - 1), with D_i = [lo(prev) - lo(i), hi(prev) - hi(i)], prev = the chain's
// row before i:
//     OR_i dilate(R_i, S_i) = dilate(R_0 | dilate(R_1 | ... dilate(R_{i0 - 1} | dilate(R_{i0}, D_{i0 - 1}), D_{i0 - 2}) ..., D_0), S_0)
// The accumulator starts at the widest row, is dilated by the small difference to the next narrower span, takes that row, and
// is dilated by the end row's own span at the end: at k = 30 most D are [0, 0] or one bit wide, 17 dilations that do anything
// and about 46 shift-ORs where the per-row form takes about 170.  A row outside the bottom region contributes zero words and
// the chain goes on.  The accumulator of row i must hold bits [64 + lo_i, 127 + hi_i] of the segment: the segment is enough
// while -63 <= lo, hi <= 63.
struct LgStemPlan {
    int nested;            // 1: the chains below apply; 0 (spans not nested): the per-row loop (lg_stem_word_rows)
    int i0;                // the widest row
    signed char dlo[64];   // row i != i0: lo of the chain's previous row - lo of row i (<= 0)
    signed char dhi[64];   //              hi of the chain's previous row - hi of row i (>= 0)
};
// nested = every row non-empty, within 63 bits, inside the chain's previous row, and 0 inside both end rows
__host__ __device__ inline void lg_make_stem_plan(const LgSeSpans& se, LgStemPlan* p) {
    p->nested = 0; p->i0 = 0;
    for (int i = 0; i < 64; i++) p->dlo[i] = p->dhi[i] = 0;
    if (se.n < 1 || se.n > 64) return;
    int i0 = 0;
    for (int i = 0; i < se.n; i++) {
        if (se.lo[i] > se.hi[i] || se.lo[i] < -63 || se.hi[i] > 63) return;
        if (se.hi[i] - se.lo[i] > se.hi[i0] - se.lo[i0]) i0 = i;
    }
    for (int i = 0; i < se.n; i++) {
        if (i == i0) continue;
        const int prev = i < i0 ? i + 1 : i - 1;
        const int dlo = se.lo[prev] - se.lo[i], dhi = se.hi[prev] - se.hi[i];
        if (dlo > 0 || dhi < 0) return;
        p->dlo[i] = (signed char)dlo; p->dhi[i] = (signed char)dhi;
    }
    if (se.lo[0] > 0 || se.hi[0] < 0 || se.lo[se.n - 1] > 0 || se.hi[se.n - 1] < 0) return;
    p->i0 = i0;
    p->nested = 1;
}
// out(p) = OR over d in [lo, hi] of a(p + d), -63 <= lo <= 0 <= hi <= 63; each side by doubling
__host__ __device__ inline LgU192 lg_dil192(LgU192 a, int lo, int hi) {
    if (!(a.w0 | a.w1 | a.w2)) return a;
    LgU192 t = a;
    if (hi > 0) {
        int covered = 1;   // t covers shifts [0, covered - 1]
        while (covered * 2 <= hi + 1) { t = lg_or192(t, lg_shr192(t, covered)); covered *= 2; }
        if (covered < hi + 1) t = lg_or192(t, lg_shr192(t, hi + 1 - covered));
    }
    if (lo < 0) {
        LgU192 l = a;
        int covered = 1;
        while (covered * 2 <= 1 - lo) { l = lg_or192(l, lg_shl192(l, covered)); covered *= 2; }
        if (covered < 1 - lo) l = lg_or192(l, lg_shl192(l, 1 - lo - covered));
        t = lg_or192(t, l);
    }
    return t;
}
__host__ __device__ inline unsigned long long lg_stem_word_chain(const unsigned long long* fb, int H, int WW, int bottom_start,
                                                                 int y, int w, const LgSeSpans& se, const LgStemPlan& pl) {
    const int y0 = y - se.anchor;
    const LgU192 r0 = lg_stem_row192(fb, H, WW, bottom_start, y0 + pl.i0, w);
    LgU192 a = r0;
    for (int i = pl.i0 - 1; i >= 0; i--)
        a = lg_or192(lg_stem_row192(fb, H, WW, bottom_start, y0 + i, w), lg_dil192(a, pl.dlo[i], pl.dhi[i]));
    unsigned long long out = lg_dil192(a, se.lo[0], se.hi[0]).w1;
    if (pl.i0 < se.n - 1) {
        a = r0;
        for (int i = pl.i0 + 1; i < se.n; i++)
            a = lg_or192(lg_stem_row192(fb, H, WW, bottom_start, y0 + i, w), lg_dil192(a, pl.dlo[i], pl.dhi[i]));
        out |= lg_dil192(a, se.lo[se.n - 1], se.hi[se.n - 1]).w1;
    }
    return out;
}
// ---- label-aware mode (lg_params.label_aware; lg_iso.hip)
// Closed-form norm of the (0.955, 1.3693) chamfer mask: with a zero pixel in the image, the two 3x3 raster passes of
// cv2.distanceTransform give min over the zero pixels q of lg_norm3(|p - q|) (a <= b <= 2a: a diagonal step never loses against
// two straight ones, and never beats one).  The device runs the raster passes themselves (lg_iso_sweep_kernel), whose integers
// are OpenCV's by construction; the norm is the independent statement of their result that the CPU tests hold to the oracle.
__host__ __device__ inline uint32_t lg_norm3(int dx, int dy) {
    const uint32_t a = (uint32_t)(dx > dy ? dx : dy), b = (uint32_t)(dx > dy ? dy : dx);
    return (a - b) * LG_A3 + b * LG_B3;
}
// One word of cv2.dilate(frame, ellipse) on bit rows: the stem code with the whole frame as its bottom region (the source-row
// fetch then zeroes only the rows outside the frame), by the chains when the spans are nested.  last_mask: the valid bits of
// the row's last word (the dilation of a pixel near the right border reaches past W; there is no pixel there).
// lg_iso_dilate_kernel and the host export lg_dilate_words_host run this code.
__host__ __device__ inline unsigned long long lg_frame_dilate_word(const unsigned long long* fb, int H, int W, int WW, int y, int w,
                                                                   const LgSeSpans& se, const LgStemPlan& pl) {
    unsigned long long o = pl.nested ? lg_stem_word_chain(fb, H, WW, 0, y, w, se, pl) : lg_stem_word_rows(fb, H, WW, 0, y, w, se);
    if (w == WW - 1 && (W & 63)) o &= ~0ull >> (64 - (W & 63));
    return o;
}
// Words per frame of the label-aware mode's `iso_mf` array (zeroed in front of the bit-row pass): [0], [1] whole-frame maxima
// of the two chamfer-3 transforms (atomicMax), [2] != 0: the frame has a pixel of another leaf, [3] unused
#define LG_ISO_MF 4
// isolation of one pixel of the current leaf from the two transforms (oracle lines 401, 404-408 in order and type: float32
// transforms, max + 1e-6 in float32 as numpy adds a Python float to a float32 scalar, the weighted sum in float32)
__host__ __device__ inline float lg_iso_value(uint32_t dc_fix, uint32_t dw_fix, uint32_t maxc, uint32_t maxw, float w_close,
                                              float w_wide, float ramp) {
#pragma clang fp contract(off)
    const float k = 1.0f / 65536.0f;
    const float sc = ((float)dc_fix * k) / ((float)maxc * k + 1e-6f);
    const float sw = ((float)dw_fix * k) / ((float)maxw * k + 1e-6f);
    return (w_close * sc + w_wide * sw) * ramp;
}

// Rows and words of a frame's stem plane that can be non-zero: the words of the mask's bounding box in the rows from which
// the ellipse reaches the bottom region.  *ya > *yb: none.
struct LgStemRect { int ya, yb, w0, w1; };   // rows [ya, yb], words [w0, w1], inclusive
__host__ __device__ inline LgStemRect lg_stem_active(const LgWin& wn, int H, int WW, int bottom_start, int se_n, int se_anchor) {
    LgStemRect r = {0, -1, 0, -1};
    if (wn.bx1 < wn.bx0 || wn.by1 < wn.by0) return r;
    const int top = bottom_start - (se_n - 1 - se_anchor);
    int ya = wn.by0 > top ? wn.by0 : top;
    if (ya < 0) ya = 0;
    const int yb = wn.by1 < H - 1 ? wn.by1 : H - 1;
    const int w0 = (wn.bx0 >> 6) > 0 ? (wn.bx0 >> 6) : 0;
    const int w1 = (wn.bx1 >> 6) < WW - 1 ? (wn.bx1 >> 6) : WW - 1;
    if (w0 > w1 || ya > yb) return r;
    r.ya = ya; r.yb = yb; r.w0 = w0; r.w1 = w1;
    return r;
}

struct LgFinalArgs {
    const float* depth;
    const unsigned long long* bits;
    const unsigned long long* stem_bits;
    const uint32_t* maxfix;       // [B][2] max fixed-point d_in / d_out
    const LgWin* win;             // [B] sweep windows
    int win_wc;                   // columns per sweep wave (64 * E)
    const LgFrameParams* fp;      // [B]
    float* maps[LG_NUM_MAPS];     // [B][H][W] each (may be null except DISTANCE/TRADITIONAL)
    uint8_t* valid;               // [B][H][W] or null
    unsigned long long* tilekeys; // [B][tiles]
    uint8_t* tile_state;          // [B][tiles] or null: 1 = the tile's planes and validity were written, 0 = constant tile
    int sparse;                   // 1: constant tiles write no plane and no validity byte (only their key and state byte)
    int score_only;               // 1 (deferred planes; with sparse): stencil tiles store traditional, validity, flatness and
                                  //   distance = 0 outside the sweep window only; lg_launch_gather computes the other five planes at its windows
    int B, H, W, WW, tiles_x, tiles_y;
    int cxi, cyi;      // floor of the optical centre; (x - cxi) is exact, the fraction is subtracted afterwards
    float cxf, cyf, f;  // fractions in [0,1) and the focal length
    float w_approach, w_sdf, w_flat, w_access;
    float sdf_w_interior, sdf_w_align, sdf_w_sdf, optimal_distance;
    float access_w_dist, access_w_dir, flat_scale;
    float iso_w_close, iso_w_wide, iso_ramp_top, iso_ramp_bottom, iso_inv_max;
    float min_edge_distance, stem_valid_thresh;
    float inv_maxd;
    uint32_t init0;    // lg_params.chamfer_init_dist0
    float inv_2s2, iso_ramp_step;   // 1 / (2 optimal_distance^2) (float32 reciprocal), (ramp_bottom - ramp_top) / (H - 1)
    float k1[7];  // separable 1-D Gaussian: 2 * gauss_r + 1 taps, sigma = size / 6 (image_processor.py:25-32)
    int gauss_r;    // radius of that Gaussian: 0..3 (lg_params.gaussian_size 1, 3, 5, 7)
    int no_skip;    // bit 0: tile-level constant path off, bit 1: wave-level off-leaf shortcut off (LG_NO_SKIP; same results, A/B timing)
    int nt_stores;  // always 0: plain plane stores (1: non-temporal, measured slower; no switch selects it any more, the kernel's text
                    // stays as measured: profiles/NOTES_options.md, section 3)
    int persist;    // from the caller, LgOptions::final_persist: resident workgroups per CU that walk the tiles (< 0: the mode's default)
    int tpw;        // > 0: consecutive tiles per workgroup (from the caller LgOptions::final_tpw; lg_launch_final leaves what the kernel reads)
    // near launch (sparse mode): the workgroups take the entries of the batch's list of near tiles (lg_near_tiles) instead of
    // every tile; the far tiles' keys and state bytes were written by lg_launch_near_tiles.  null: every tile
    const int32_t* near_off;   // [B + 1] DEVICE: first list entry of every frame, near_off[B] = near_total
    int near_total;            // entries of the list (the host's copy of near_off[B])
    int near_tpw;              // consecutive list entries per workgroup (>= 1)
};

// kernel launchers (lg_kernels.hip)
// mf (null: bit rows only): the frames' maxfix words, zeroed by the caller: the pass adds every frame's bounding box and area
// to mf[b * LG_MF + LG_BOX_X0 ..] (see LG_MF), at most five integer atomics per workgroup that saw a set bit
void lg_launch_pack_bits(const uint8_t* mask, unsigned long long* bits, int B, int H, int W, int WW, hipStream_t s,
                         uint32_t* mf = nullptr);
// mask[b] = labels[b] == ids[b] (0 / 1 bytes) and its bit rows in one pass (ids: DEVICE, one per frame)
// others / iso_mf (label-aware mode; both or neither): also the bit rows of others[b] = labels[b] > 0 && labels[b] != ids[b], in
// the same read of the labels, and iso_mf[b * LG_ISO_MF + 2] != 0 for a frame that has such a pixel (iso_mf zeroed by the caller)
void lg_launch_pack_labels(const int16_t* labels, const int32_t* ids_dev, uint8_t* mask, unsigned long long* bits, int B, int H,
                           int W, int WW, hipStream_t s, uint32_t* mf = nullptr, unsigned long long* others = nullptr,
                           uint32_t* iso_mf = nullptr);
void lg_launch_export_rows(const unsigned long long* bits, const LgWin* wins, unsigned long long* dst_host_devptr, int B,
                           int H, int WW, hipStream_t s);
// plan (lg_make_stem_plan of se) nested and wins given: the nested-span kernel on the frames' bounding boxes; else the per-row kernel
void lg_launch_stem_bits(const unsigned long long* bits, unsigned long long* stem, const LgWin* wins, int B, int H, int W, int WW,
                         int bottom_start, const LgSeSpans& se, const LgStemPlan* plan, hipStream_t s);
void lg_launch_final(const LgFinalArgs& a, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// Near tiles of a batch, in front of the near launch of lg_final_kernel (LgFinalArgs::near_off): near_off[b] = near tiles of the
// frames before b (exclusive scan of lg_near_tiles over win[0 .. B), near_off[B] = their total), and every FAR tile's constant
// key and state byte 0 into tilekeys / tile_state -- exactly what lg_final_kernel's constant path stores.  No atomics: the
// same output on every run.  halo: Gaussian radius + 1 of the plane kernel that follows.  near_off_host_dev (or null): the
// device alias of the host's pinned copy of near_off, which the kernel then writes as well.
void lg_launch_near_tiles(const LgWin* win, int B, int H, int W, int halo, int32_t* near_off, int32_t* near_off_host_dev,
                          unsigned long long* tilekeys, uint8_t* tile_state, hipStream_t s);
void lg_launch_smooth(const float* src, float* dst, int B, int H, int W, int S, const LgGaussTaps& taps, hipStream_t s);
// tile_state (sparse planes, LgFinalArgs::sparse): [B][tiles] from lg_final_kernel, null when every plane was written.  The
// planes of a tile with state 0 were not written: top-k and the gather use the constant tile's values instead (flat_scale,
// w_flat: lg_params), computed with the operations of the final kernel's constant path.
// keep (needs out_info): [B] bit i = candidate i is scored by the rescoring and can still win (see lg_launch_survivors).
void lg_launch_topk(const float* trad, const uint8_t* valid, const float* depth, unsigned long long* tilekeys,
                    const uint8_t* tile_state, float flat_scale, float w_flat,
                    bool keys_ready, int B, int H, int W, int k, int min_dist, int32_t* out_xy, int32_t* out_n,
                    float* out_info, hipStream_t s, unsigned long long* keep = nullptr, int mask_is_bool = 0);
// list / count (lg_launch_survivors; both null: every candidate): patch slot j takes entry list[j], slots >= *count are left alone
// defer (deferred planes; haloed patches, tile_state given): the arguments of the score-only lg_launch_final over the same
// frames.  Of maps_dev only flatness and distance are read then; sdf, approach, isolation, accessibility and stem of a window's
// pixels on a state-1 tile are computed here, by the plane kernel's own per-pixel code.
void lg_launch_gather(const float* depth, const uint8_t* mask, const float* const* maps_dev, const uint8_t* tile_state,
                      float flat_scale, int B, int H, int W, int k, const int32_t* xy, const int32_t* n, float* patches,
                      bool haloed, hipStream_t s, const int32_t* list = nullptr, const int32_t* count = nullptr,
                      const LgFinalArgs* defer = nullptr, const struct LgIsoFields* iso = nullptr);

// ---- label-aware isolation (lg_iso.hip), every launch over the frames [0, B) of its pointers
// The two transforms of a batch and where the deferred gather / the plane kernel find them.  A frame with iso_mf[.. + 2] == 0
// (no other leaf) is skipped by every kernel: its plane stays the closed form.
struct LgIsoFields {
    const uint32_t* fields;   // [B][2][H][W] 16.16 transforms of 1 - ic (0) and 1 - iw (1)
    const uint32_t* iso_mf;   // [B][LG_ISO_MF]
};
// the generic-width companion of lg_launch_pack_labels: others' bit rows and flag alone, one wave ballot per word
void lg_launch_pack_others(const int16_t* labels, const int32_t* ids_dev, unsigned long long* others, uint32_t* iso_mf, int B, int H,
                           int W, int WW, hipStream_t s);
// dil[0][b] = dilate(others[b], ellipse 30), dil[1][b] = dilate(others[b], ellipse 40) as bit rows (dil: [2][B][H][WW])
void lg_launch_iso_dilate(const unsigned long long* others, unsigned long long* dil, const uint32_t* iso_mf, int B, int H, int W, int WW,
                          hipStream_t s);
// The 3x3 raster passes of cv2.distanceTransform(1 - dil[f][b], DIST_L2, 3) into fields[b][f], forward then backward (two
// launches), and the whole-frame maxima into iso_mf[b][f].  0: queued, -1: width not supported (W > 8192)
int lg_launch_iso_sweeps(const unsigned long long* dil, uint32_t* fields, uint32_t* iso_mf, int B, int H, int W, int WW, uint32_t init0,
                         hipStream_t s);
// dense planes: isolation[b] on the pixels of the current leaf (bit rows `bits`, bounding boxes `win`) from the fields
void lg_launch_iso_plane(const LgIsoFields& f, const unsigned long long* bits, const LgWin* win, float* iso, int B, int H, int W, int WW,
                         float w_close, float w_wide, float ramp_top, float ramp_step, hipStream_t s);

// The host half of select_grasp_point on the device (lg_finish_kernel): CNN rescoring of the candidates, 3-D point, pre-grasp point
struct LgFinishArgs {
    const int32_t* cand_n;        // [B]
    const int32_t* cand_xy;       // [B][K][2]
    const float* cand_info;       // [B][K][2] traditional score, depth at the candidate
    const float* logits;          // [B][K] (read only when use_cnn); with `slot`: one per patch slot
    const int32_t* slot;          // [B][K] patch slot of a candidate, -1: pruned (lg_launch_survivors); null: slot = b * K + i
    int slot_frames;              //   slots count from the first patch of the candidate's sub-batch of this many frames
    const LgFrameParams* fp;      // [B] (theta)
    const unsigned long long* bits;   // [B][H][WW] mask bit rows
    const unsigned long long* bits2;  // null, or (label-aware mode) [B][H][WW] bit rows of the other leaves: the pre-grasp probes
                                      //   test bits | bits2 = every leaf of the label image
    lg_grasp_result* out;         // [B] DEVICE
    int B, H, W, WW, K, use_cnn, mask_is_bool;
    double cx, cy, f;
    LgSeSpans se;                 // (2 * pregrasp_clearance + 1) ellipse
};
void lg_launch_finish(const LgFinishArgs& a, hipStream_t s);
// Every candidate of every frame in rank order (lg_candidates_kernel, after lg_launch_finish on the same stream): rows [B][K]
void lg_launch_candidates(const LgFinishArgs& a, lg_grasp_candidate* rows, hipStream_t s);

// The reference's selection (grasp_point_selector.py:205-236) applied again to what is left after each pick: remaining = 0..n-1
// in candidate order; rank r starts from the first remaining candidate j with best score trad[j] and, when rescoring and more
// than one candidate remains, takes every scored remaining i with comb[i] > best (in candidate order); the pick leaves the
// list.  Rank 0 is the reference's grasp point.  Comparisons only, as written: a NaN never wins and a NaN start is never
// beaten.  n <= 64.  The device (lg_candidates_kernel) and the host export lg_rank_grasp_candidates run this code.
__host__ __device__ inline void lg_rank_candidates(const double* trad, const double* comb, const int32_t* scored, int n,
                                                   int rescoring, int32_t* order, double* pick, int32_t* by_ml) {
    unsigned long long left = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    for (int r = 0; r < n; r++) {
        const int j = __builtin_ctzll(left);
        int best = j, ml = 0;
        double bs = trad[j];                                   // :205-207
        if (rescoring && (left & (left - 1ull)) != 0ull)      // :210, len(candidates) > 1
            for (unsigned long long m = left; m; m &= m - 1ull) {
                const int i = __builtin_ctzll(m);
                if (scored[i] && comb[i] > bs) { bs = comb[i]; best = i; ml = 1; }   // :226-236
            }
        order[r] = best;
        pick[r] = bs;
        by_ml[r] = ml;
        left &= ~(1ull << best);
    }
}

// CNN rescoring of one candidate (grasp_point_selector.py:133-136, :222-226): ml = tanh(3 sigmoid(logit)) / 2 + 1/2, its
// confidence, weight and combined score, in float64 with fp contraction off.  lg_finish_kernel / lg_candidates_kernel
// (lg_ml_rescore) and the host export lg_ml_combined_score run this code.
__host__ __device__ inline void lg_ml_combine(double logit, double trad, double* ml_out, double* conf_out, double* comb_out) {
#pragma clang fp contract(off)
    const double sg = 1.0 / (1.0 + exp(-logit));
    const double ml = tanh(sg * 3.0) * 0.5 + 0.5;               // :133-136
    const double conf = 1.0 - fabs(ml - 0.5) * 2.0;              // :222
    const double wml = fmin(0.3, conf * 0.6);                    // :223
    *comb_out = (1.0 - wml) * trad + wml * ml;                   // :226
    *ml_out = ml;
    *conf_out = conf;
}

// true: a candidate with traditional score trad_i can never be taken by the selection loop (:226-236) of a frame whose
// candidate 0 has traditional score trad_0, whatever its logit -- its patch need not go through the CNN.  The loop starts
// from best = trad_0 and takes i only if comb_i > best, and best never falls.  ml lies in [0.5, 1]; maximising comb over ml:
//   trad_i <  0.5: w = 0.3 up to ml = 0.75, falling behind it      -> comb <= 0.7 trad_i + 0.225          (at ml = 0.75)
//   trad_i >= 0.5: w = 1.2 (1 - ml) behind 0.75, vertex (1 + t) / 2 -> comb <= trad_i + 0.3 (1 - trad_i)^2 (trad_i >= 1: comb <= trad_i)
// The margin covers the rounding of the float64 comb chain (a few ulp of 1 + |trad|; the margin is a thousand times that,
// float32 scores lie 6e-8 apart).  A NaN or an infinity in either score keeps the candidate.
__host__ __device__ inline bool lg_cnn_cannot_win(double trad_i, double trad_0) {
#pragma clang fp contract(off)
    if (!(fabs(trad_i) <= 1.7976931348623157e308) || !(fabs(trad_0) <= 1.7976931348623157e308)) return false;
    const double d = 1.0 - trad_i;
    const double ub = trad_i < 0.5 ? 0.7 * trad_i + 0.225 : trad_i + 0.3 * (d * d);
    const double margin = 1e-12 * (1.0 + fabs(trad_0) + fabs(trad_i));
    return ub + margin <= trad_0;
}

// Survivors of a batch (lg_launch_survivors, after lg_launch_topk with `keep`): keep[b] = bit i set when candidate i of frame
// b is scored by the rescoring (n > 1, border rule of a torch.bool mask) and can still win (lg_cnn_cannot_win).  list[j] =
// b * K + i of the j-th set bit in (frame, candidate) order, *count = their number, slot[b * K + i] = j or -1.  One workgroup;
// no atomics: the list is the same on every run.
void lg_launch_survivors(const unsigned long long* keep, int B, int K, int32_t* list, int32_t* slot, int32_t* count, hipStream_t s);

// host-side contour analysis on the bit-packed mask (lg_contour.cpp)
// returns 1 and fills out[0..4] = angle(rad,(0,pi]), major, minor, cx, cy ; 0 if the mask is empty
int lg_host_orientation(const unsigned long long* bits, int H, int W, int WW, double* out);
// the same on the band of rows [y_off, y_off + H) (bits -> row y_off); results in absolute image coordinates
int lg_host_orientation_rows(const unsigned long long* bits, int H, int W, int WW, int y_off, double* out);
// ... and reading only the words [w0, w1] of every row (all other pixels are empty)
int lg_host_orientation_band(const unsigned long long* bits, int H, int W, int WW, int y_off, int w0, int w1, double* out);
// 1 if any set bit of `bits` lies under the (2c+1)^2 ellipse centred at (u,v)  (pre-grasp clearance probe)
int lg_host_ellipse_hit(const unsigned long long* bits, int H, int W, int WW, int u, int v, int clearance);
int lg_host_ellipse_hit_se(const unsigned long long* bits, int H, int W, int WW, int u, int v, const LgSeSpans& se);
int lg_host_ellipse_hit_band(const unsigned long long* bits, int H, int W, int WW, int w0, int w1, int u, int v,
                             const LgSeSpans& se);
void lg_make_se_spans(int k, LgSeSpans* out);
#ifdef __cplusplus
#include <vector>
// outer contour (all border pixels, tracing order) of the component with the largest contour area; returns #points
int lg_host_contour_points(const unsigned long long* bits, int H, int W, int WW, std::vector<int>& xy);
#endif
void lg_launch_harvest(const float* depth, const uint8_t* mask, const float* const* maps_host, int H, int W, int n,
                       const int32_t* xy, const int32_t* rot, float* out_depth, float* out_mask, float* out_scores,
                       int32_t* flags, hipStream_t s);
void lg_launch_negative_masks(const float* dist, const uint8_t* mask, uint8_t* tip, uint8_t* stem, uint8_t* scratch, int H,
                              int W, hipStream_t s);
