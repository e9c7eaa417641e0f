// Bit rows (lg_bits.hip): 192-bit segments of them and the stem dilation on those (also behind lg_iso.hip's dilation), the
// active rectangle of a stem plane, the plane kernel's wave-level mask test, and the launchers of the bit-row pass.
#pragma once
#include "lg_internal.h"

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

// ---- launchers (lg_bits.hip)
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
