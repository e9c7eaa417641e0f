// ML-only grasp selection, the device-side link between the bit rows and the gather / CNN / finish kernels (lg_mlsel.h):
// row counts -> sample table -> slot list -> (gather + CNN in chunks, lg_select.hip) -> pick -> (lg_finish_kernel) -> result rows.
// Every step is a launch of its own; nothing here waits on another workgroup.  Integer counts, 64-wide scans and no atomics:
// the table and the list are the same on every run.
#include "lg_internal.h"
#include "lg_mlsel.h"

namespace {

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of NT threads (NT / 64 waves); *total = the sum.  s_w: NT / 64 + 1 ints.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int t, int* s_w, int* total) {
    const int lane = t & 63, wv = t >> 6;
    const int inc = wave_incl_scan(v, lane);
    __syncthreads();   // (s_w's readers of the round before are done)
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        const int c = s_w[i];
        if (i < wv) base += c;
        sum += c;
    }
    *total = sum;
    return base + inc - v;
}

// One workgroup per frame.  A group of L lanes (L = the power of two that covers the box's words, at most 64) takes one row:
// neighbouring lanes read neighbouring words.  Per row: the pixels a sample can sit on; per frame: area, sum of x, sum of y.
// Then the exclusive prefix over the rows, 256 at a time with a running base.
__global__ __launch_bounds__(256) void lg_ml_rows_kernel(const unsigned long long* __restrict__ bits, const LgWin* __restrict__ win,
                                                         lg_ml_sampling s, LgMlBuffers m, int H, int W, int WW) {
    __shared__ unsigned long long s_pat[128];   // W <= 8192
    __shared__ long long s_red[3][4];
    __shared__ int s_w[5];
    const int b = blockIdx.x, t = threadIdx.x;
    const LgWin wn = win[b];
    LgMlFrame f;
    f.sx = 0; f.sy = 0; f.area = 0; f.total = 0; f.step = 1; f.n = 0; f.y0 = 0; f.rows = 0; f.w0 = 0; f.w1 = -1; f.n_scored = 0; f.pad_ = 0;
    if (wn.bx1 < wn.bx0 || wn.by1 < wn.by0 || wn.area <= 0) {   // empty mask
        if (t == 0) { m.frames[b] = f; m.counts[2 * b] = 0; m.counts[2 * b + 1] = 0; m.n_frame[b] = 0; }
        return;
    }
    f.y0 = max(wn.by0, 0); f.rows = min(wn.by1, H - 1) - f.y0 + 1;
    f.w0 = max(wn.bx0 >> 6, 0); f.w1 = min(wn.bx1 >> 6, WW - 1);
    for (int w = t; w < WW && w < 128; w += 256) s_pat[w] = lg_ml_pattern(s.mode, s.stride, w);
    __syncthreads();
    const unsigned long long* fb = bits + (size_t)b * H * WW;
    int32_t* pre = m.row_pre + (size_t)b * H;
    const int nw = f.w1 - f.w0 + 1;
    int L = 1;
    while (L < nw && L < 64) L <<= 1;
    const int R = 256 / L, g = t & (L - 1), gr = t / L;
    long long acc_a = 0, acc_x = 0, acc_y = 0;
    for (int r0 = 0; r0 < f.rows; r0 += R) {
        const int ry = r0 + gr;
        int cnt = 0, ar = 0;
        long long sx = 0;
        if (ry < f.rows) {
            const int y = f.y0 + ry;
            const bool on = lg_ml_row_sampled(s.mode, s.stride, y);
            const unsigned long long* row = fb + (size_t)y * WW;
            for (int w = f.w0 + g; w <= f.w1; w += L) {
                const unsigned long long v = row[w];
                const int c = __popcll(v);
                ar += c;
                sx += (long long)c * (64 * w) + lg_ml_index_sum(v);
                if (on) cnt += __popcll(v & s_pat[w]);
            }
        }
        for (int o = L >> 1; o >= 1; o >>= 1) {   // (L <= 64: a group never spans two waves)
            cnt += __shfl_xor(cnt, o, 64);
            ar += __shfl_xor(ar, o, 64);
            sx += __shfl_xor(sx, o, 64);
        }
        if (g == 0 && ry < f.rows) {
            pre[ry] = cnt;
            acc_a += ar; acc_x += sx; acc_y += (long long)ar * (f.y0 + ry);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc_a += __shfl_xor(acc_a, o, 64);
        acc_x += __shfl_xor(acc_x, o, 64);
        acc_y += __shfl_xor(acc_y, o, 64);
    }
    if ((t & 63) == 0) { s_red[0][t >> 6] = acc_a; s_red[1][t >> 6] = acc_x; s_red[2][t >> 6] = acc_y; }
    __syncthreads();   // (also: the row counts written above are visible to the whole workgroup)
    f.area = (int)(s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]);
    f.sx = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    f.sy = s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3];
    int base = 0;
    for (int r0 = 0; r0 < f.rows; r0 += 256) {
        const int ry = r0 + t;
        const int c = ry < f.rows ? pre[ry] : 0;
        int tot;
        const int ex = block_excl_scan<256>(c, t, s_w, &tot);
        if (ry < f.rows) pre[ry] = base + ex;
        base += tot;
    }
    f.total = base;
    lg_ml_frame_counts(s, &f);
    if (t == 0) { m.frames[b] = f; m.counts[2 * b] = f.n; m.n_frame[b] = f.n > 0 ? f.n : 0; }
}

// One workgroup per frame, one thread per sample index, 1024 at a time: the sample's pixel (lg_ml_locate), whether it is scored,
// and a scored sample's rank among the frame's scored samples (running base over the rounds).
__global__ __launch_bounds__(1024) void lg_ml_table_kernel(const unsigned long long* __restrict__ bits, lg_ml_sampling s, LgMlBuffers m,
                                                           int H, int W, int WW) {
    __shared__ int s_w[17];
    const int b = blockIdx.x, t = threadIdx.x, M = s.max_samples;
    const LgMlFrame f = m.frames[b];
    const int n = f.n > 0 ? (f.n < M ? f.n : M) : 0;   // (an overflowed frame has no table)
    const unsigned long long* fb = bits + (size_t)b * H * WW;
    const int32_t* pre = m.row_pre + (size_t)b * H;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + t;
        int x = 0, y = 0, sc = 0;
        if (i < n) lg_ml_locate(fb, H, W, WW, s, f, pre, i, &x, &y, &sc);
        int tot;
        const int ex = block_excl_scan<1024>(sc, t, s_w, &tot);
        if (i < n) {
            const size_t o = (size_t)b * M + i;
            m.xy[2 * o] = x; m.xy[2 * o + 1] = y;
            m.scored[o] = sc;
            m.slot_local[o] = sc ? base + ex : -1;
        }
        base += tot;
    }
    if (t == 0) { m.frames[b].n_scored = base; m.counts[2 * b + 1] = base; }
}

// list[first slot of the frame + rank] = frame * M + sample and its inverse.  The frame's first slot = the scored samples of the
// frames before it, summed by every workgroup for itself (B integers).
__global__ __launch_bounds__(256) void lg_ml_list_kernel(LgMlBuffers m, int M, int B) {
    __shared__ int s_part[4], s_off;
    const int b = blockIdx.y, t = threadIdx.x;
    int part = 0;
    for (int k = t; k < b; k += 256) part += m.counts[2 * k + 1];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((t & 63) == 0) s_part[t >> 6] = part;
    __syncthreads();
    if (t == 0) s_off = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();
    const int n = m.counts[2 * b];
    const int i = blockIdx.x * 256 + t;
    if (i >= M) return;
    const size_t o = (size_t)b * M + i;
    int sl = -1;
    if (i < n && m.slot_local[o] >= 0) {
        sl = s_off + m.slot_local[o];
        m.list[sl] = (int32_t)o;
    }
    m.slot[o] = sl;
}

// One workgroup per frame.  The pick is the first sample, in table order, whose logit is greater than every earlier scored
// sample's -- the first occurrence of the largest logit that is not a NaN (:364, score > best_score).  Without one: the centroid
// of the mask from the exact integer sums, truncated (:368-378).
__global__ __launch_bounds__(256) void lg_ml_pick_kernel(const float* __restrict__ depth, LgMlBuffers m, int M, int H, int W, int has_logits) {
#pragma clang fp contract(off)
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const LgMlFrame f = m.frames[b];
    const int n = f.n > 0 ? (f.n < M ? f.n : M) : 0;
    float bv = 0.0f;
    int bi = -1;
    if (has_logits)
        for (int i = t; i < n; i += 256) {   // (a thread's indices ascend: strictly greater keeps its first maximum)
            const int sl = m.slot[(size_t)b * M + i];
            if (sl < 0) continue;
            const float v = m.logits[sl];
            if (v != v) continue;
            if (bi < 0 || v > bv) { bv = v; bi = i; }
        }
    auto better = [](float v, int i, float bv_, int bi_) { return i >= 0 && (bi_ < 0 || v > bv_ || (v == bv_ && i < bi_)); };
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((t & 63) == 0) { s_v[t >> 6] = bv; s_i[t >> 6] = bi; }
    __syncthreads();
    if (t != 0) return;
    for (int k = 1; k < 4; k++)
        if (better(s_v[k], s_i[k], bv, bi)) { bv = s_v[k]; bi = s_i[k]; }
    int found = 0, x = 0, y = 0, ml_used = 0;
    float ml_f = __builtin_nanf("");
    if (f.area > 0 && f.n >= 0) {   // (an empty mask and an overflowed GRID frame: found = 0)
        found = 1;
        if (bi >= 0) {
            x = m.xy[2 * ((size_t)b * M + bi)]; y = m.xy[2 * ((size_t)b * M + bi) + 1];
            double ml, conf, comb;
            lg_ml_combine((double)bv, 0.0, &ml, &conf, &comb);
            ml_f = (float)ml;
            ml_used = 1;
        } else {
            x = (int)(f.sx / f.area); y = (int)(f.sy / f.area);
        }
    }
    m.pick_n[b] = found;
    m.pick_xy[2 * b] = x; m.pick_xy[2 * b + 1] = y;
    m.pick_info[2 * b] = 0.0f;
    m.pick_info[2 * b + 1] = found ? depth[(size_t)b * H * W + (size_t)y * W + x] : 0.0f;
    m.pick_meta[4 * b] = ml_used;
    m.pick_meta[4 * b + 1] = has_logits ? f.n_scored : 0;   // (samples that went through the CNN)
    m.pick_meta[4 * b + 2] = __float_as_int(ml_f);
    m.pick_meta[4 * b + 3] = 0;
}

// Behind lg_finish_kernel: the three fields of the result row that mean something else here, and the lg_ml_sample rows.
__global__ __launch_bounds__(256) void lg_ml_rows_out_kernel(LgMlBuffers m, int M, int has_logits, lg_grasp_result* __restrict__ res,
                                                             lg_ml_sample* __restrict__ rows) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, t = threadIdx.x;
    const int i = blockIdx.x * 256 + t;
    if (i == 0) {
        res[b].n_candidates = m.pick_meta[4 * b + 1];
        res[b].ml_used = m.pick_meta[4 * b];
        res[b].best_score = __int_as_float(m.pick_meta[4 * b + 2]);
    }
    if (!rows || i >= M) return;
    const int n = m.counts[2 * b];
    const size_t o = (size_t)b * M + i;
    lg_ml_sample r;
    r.x = 0; r.y = 0; r.scored = 0; r.logit = 0.0f; r.ml_score = 0.0f;   // rows past the frame's samples: zeros
    if (i < n) {
        r.x = m.xy[2 * o]; r.y = m.xy[2 * o + 1];
        const int sl = m.slot[o];
        r.scored = (sl >= 0 && has_logits) ? 1 : 0;
        r.logit = r.ml_score = __builtin_nanf("");
        if (r.scored) {
            r.logit = m.logits[sl];
            double ml, conf, comb;
            lg_ml_combine((double)r.logit, 0.0, &ml, &conf, &comb);
            r.ml_score = (float)ml;
        }
    }
    rows[o] = r;
}

}  // namespace

void lg_launch_ml_rows(const unsigned long long* bits, const LgWin* win, const lg_ml_sampling& s, const LgMlBuffers& m, int B, int H, int W,
                       int WW, hipStream_t st) {
    hipLaunchKernelGGL(lg_ml_rows_kernel, dim3(B), dim3(256), 0, st, bits, win, s, m, H, W, WW);
}
void lg_launch_ml_table(const unsigned long long* bits, const lg_ml_sampling& s, const LgMlBuffers& m, int B, int H, int W, int WW,
                        hipStream_t st) {
    hipLaunchKernelGGL(lg_ml_table_kernel, dim3(B), dim3(1024), 0, st, bits, s, m, H, W, WW);
}
void lg_launch_ml_list(const lg_ml_sampling& s, const LgMlBuffers& m, int B, hipStream_t st) {
    hipLaunchKernelGGL(lg_ml_list_kernel, dim3((s.max_samples + 255) / 256, B), dim3(256), 0, st, m, s.max_samples, B);
}
void lg_launch_ml_pick(const float* depth, const LgMlBuffers& m, int M, int B, int H, int W, int has_logits, hipStream_t st) {
    hipLaunchKernelGGL(lg_ml_pick_kernel, dim3(B), dim3(256), 0, st, depth, m, M, H, W, has_logits);
}
void lg_launch_ml_rows_out(const LgMlBuffers& m, int M, int B, int has_logits, lg_grasp_result* res, lg_ml_sample* rows, hipStream_t st) {
    hipLaunchKernelGGL(lg_ml_rows_out_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, m, M, has_logits, res, rows);
}
