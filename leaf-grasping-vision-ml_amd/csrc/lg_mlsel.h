// ML-only grasp selection (lg_select_grasp_ml*; reference scripts/utils/grasp_point_selector.py:290-390): the sample table of a
// frame from its mask bit rows, stated once for the device kernels (lg_mlsel.hip) and the host export lg_ml_sample_points_host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/leafgrasp.h"

#define LG_ML_MAX_SAMPLES 65536
#define LG_ML_DEFAULT_CHUNK 1024   // patches per gather + CNN pass (0.8 MB of activations per patch)
#define LG_ML_MAX_CHUNK 8192       // one slice of lg_cnn_run

// NULL message: the sampling is usable.  NTH needs room for its 2 target - 1 samples (it cannot overflow); GRID overflows per frame.
__host__ __device__ inline const char* lg_ml_sampling_error(const lg_ml_sampling* s) {
    if (!s) return "sampling is null";
    if (s->mode != LG_ML_SAMPLE_NTH && s->mode != LG_ML_SAMPLE_GRID) return "sampling mode must be LG_ML_SAMPLE_NTH or LG_ML_SAMPLE_GRID";
    if (s->max_samples < 1 || s->max_samples > LG_ML_MAX_SAMPLES) return "max_samples must be in [1, 65536]";
    if (s->chunk < 0 || s->chunk > LG_ML_MAX_CHUNK) return "chunk must be in [0, 8192]";
    if (s->mode == LG_ML_SAMPLE_NTH) {
        if (s->target < 1 || s->target > LG_ML_MAX_SAMPLES / 2) return "target must be in [1, 32768]";
        if (2 * s->target - 1 > s->max_samples) return "max_samples must hold the 2 * target - 1 samples of LG_ML_SAMPLE_NTH";
    } else if (s->stride < 1 || s->stride > 64) {
        return "stride must be in [1, 64]";
    }
    return nullptr;
}

// Bits of word w (pixels 64 w .. 64 w + 63) a sample can sit on: every bit (NTH), or the columns x % stride == 0 (GRID).  The
// first such column of the word, then copies of it stride, 2 stride, 4 stride, ... further on (a shift past bit 63 drops out).
__host__ __device__ inline unsigned long long lg_ml_pattern(int mode, int stride, int w) {
    if (mode != LG_ML_SAMPLE_GRID || stride <= 1) return ~0ull;
    const int first = (stride - (int)(((long long)w * 64) % stride)) % stride;
    unsigned long long p = 1ull << first;   // first <= stride - 1 <= 63
    for (int span = stride; span < 64; span *= 2) p |= p << span;
    return p;
}
// rows a sample can sit on
__host__ __device__ inline bool lg_ml_row_sampled(int mode, int stride, int y) {
    return mode != LG_ML_SAMPLE_GRID || stride <= 1 || y % stride == 0;
}
__host__ __device__ inline int lg_ml_popc(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
// sum of the indices of the set bits of v: bit k of an index counts 2^k for every set bit whose index has it
__host__ __device__ inline int lg_ml_index_sum(unsigned long long v) {
    return lg_ml_popc(v & 0xAAAAAAAAAAAAAAAAull) + 2 * lg_ml_popc(v & 0xCCCCCCCCCCCCCCCCull) + 4 * lg_ml_popc(v & 0xF0F0F0F0F0F0F0F0ull) +
           8 * lg_ml_popc(v & 0xFF00FF00FF00FF00ull) + 16 * lg_ml_popc(v & 0xFFFF0000FFFF0000ull) + 32 * lg_ml_popc(v & 0xFFFFFFFF00000000ull);
}
// index of the r-th set bit of v (r counts from 0, r < popcount(v)): halving search on the popcounts of the low parts
__host__ __device__ inline int lg_ml_select_bit(unsigned long long v, int r) {
    int pos = 0;
    for (int half = 32; half >= 1; half >>= 1) {
        const int c = lg_ml_popc(v & ((1ull << half) - 1ull));
        if (r >= c) { r -= c; v >>= half; pos += half; }
    }
    return pos;
}

// What the row pass leaves of one frame, all exact integers.
struct LgMlFrame {
    long long sx, sy;   // sum of x, sum of y over the set pixels (the centroid's numerators)
    int area;           // set pixels
    int total;          // pixels a sample can sit on: area (NTH), the set pixels on the stride grid (GRID)
    int step;           // NTH: max(1, area / target); GRID: 1
    int n;              // samples of the frame; GRID overflow: -(total), and no table
    int y0, rows;       // rows [y0, y0 + rows) hold every set pixel (the bounding box); rows = 0: empty mask
    int w0, w1;         // words [w0, w1] of those rows likewise
    int n_scored;       // samples off the 16-pixel border band (lg_ml_table_kernel)
    int pad_;
};
// step, n and the overflow code from the counts
__host__ __device__ inline void lg_ml_frame_counts(const lg_ml_sampling& s, LgMlFrame* f) {
    if (s.mode == LG_ML_SAMPLE_NTH) {
        const int step = f->area / s.target > 1 ? f->area / s.target : 1;   // :310  step = max(1, n // target)
        f->step = step;
        f->n = (f->total + step - 1) / step;                                 // pixels 0, step, 2 step, ... below n
    } else {
        f->step = 1;
        f->n = f->total > s.max_samples ? -f->total : f->total;
    }
}
// Sample i of a frame: leaf pixel number i * step in row-major order among the pixels a sample can sit on.  row_pre[y - y0] =
// such pixels in the rows before y (exclusive prefix over the box rows).  The row by bisection, the word by a walk over the
// row's words, the bit by lg_ml_select_bit.  scored: off the border band, :326-328 (x == W - 16 is in the band).
__host__ __device__ inline void lg_ml_locate(const unsigned long long* bits, int H, int W, int WW, const lg_ml_sampling& s,
                                             const LgMlFrame& f, const int32_t* row_pre, int i, int* x_out, int* y_out, int* scored) {
    int r = i * f.step;
    int lo = 0, hi = f.rows - 1;   // the last row whose prefix is <= r (it holds pixel r: r < total)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_pre[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int y = f.y0 + lo;
    r -= row_pre[lo];
    const unsigned long long* row = bits + (size_t)y * WW;
    int x = 0;
    for (int w = f.w0; w <= f.w1; w++) {
        const unsigned long long v = row[w] & lg_ml_pattern(s.mode, s.stride, w);
        const int c = lg_ml_popc(v);
        if (r < c) { x = 64 * w + lg_ml_select_bit(v, r); break; }
        r -= c;
    }
    *x_out = x; *y_out = y;
    *scored = (y < 16 || y >= H - 16 || x < 16 || x >= W - 16) ? 0 : 1;
}

// ---- device side (lg_mlsel.hip).  M = lg_ml_sampling.max_samples, the row length of every per-sample array.
struct LgWin;
struct LgMlBuffers {
    LgMlFrame* frames;      // [B]
    int32_t* row_pre;       // [B][H] exclusive row prefix, entries [0, rows) of a frame used
    int32_t* xy;            // [B][M][2] the table in the gather's point layout
    int32_t* scored;        // [B][M]
    int32_t* slot_local;    // [B][M] rank of a scored sample among its frame's scored samples, -1: not scored
    int32_t* list;          // [B * M] patch slot -> frame * M + sample, scored samples in (frame, sample) order
    int32_t* slot;          // [B][M] sample -> patch slot, -1: not scored
    int32_t* counts;        // [B][2] n (GRID overflow: -needed), n_scored per frame (the host reads a copy)
    int32_t* n_frame;       // [B] rows of the frame's table, max(n, 0): the gather's per-frame point count
    float* logits;          // [B * M] by patch slot
    int32_t* pick_n;        // [B]       one-candidate list for lg_launch_finish: 1, or 0 where nothing is found
    int32_t* pick_xy;       // [B][2]
    float* pick_info;       // [B][2]    (unused score, depth at the pick)
    int32_t* pick_meta;     // [B][4]    ml_used, n_scored, float bits of ml_score, unused
};
// Row counts, their exclusive prefix, sums and the frame's sample count; one workgroup per frame over its bounding-box rows.
void lg_launch_ml_rows(const unsigned long long* bits, const LgWin* win, const lg_ml_sampling& s, const LgMlBuffers& m, int B, int H, int W,
                       int WW, hipStream_t st);
// The table: one thread per sample index (a workgroup per frame walks its samples 1024 at a time), the scored samples' ranks.
void lg_launch_ml_table(const unsigned long long* bits, const lg_ml_sampling& s, const LgMlBuffers& m, int B, int H, int W, int WW,
                        hipStream_t st);
// list / slot over the whole batch from the per-frame ranks and counts
void lg_launch_ml_list(const lg_ml_sampling& s, const LgMlBuffers& m, int B, hipStream_t st);
// First-max of the logits in table order (a NaN never wins), or the centroid; fills the one-candidate list.  has_logits = 0: no model.
void lg_launch_ml_pick(const float* depth, const LgMlBuffers& m, int M, int B, int H, int W, int has_logits, hipStream_t st);
// After lg_launch_finish: n_candidates, ml_used and best_score of the result rows; the lg_ml_sample rows (rows: [B][M] DEVICE or null).
void lg_launch_ml_rows_out(const LgMlBuffers& m, int M, int B, int has_logits, lg_grasp_result* res, lg_ml_sample* rows, hipStream_t st);
