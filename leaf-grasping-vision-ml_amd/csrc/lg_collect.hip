// gfx950 kernels of the collecting selector (lg_collect.h; include/leafgrasp.h lg_select_grasp_collect):
// ellipse erosion on complemented bit rows, the tip-penalty plane as written, the variant's fusion with its per-frame
// first-maximum reduction, and the pick (arg-max, or the centroid of the original mask).  Reference semantics:
// scripts/utils/grasp_point_selector_bkp.py:73-169, :395-408.
#include "lg_collect.h"

#include <algorithm>

namespace {

__device__ __forceinline__ unsigned long long lg_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long lg_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// ============================================================================ erosion
// One thread per word.  c_0 and, in the same read, the centroid numerators of the mask: sum x, sum y and the pixel count as
// 64-bit integer sums (one atomic per wave that saw a set bit).
__global__ __launch_bounds__(256) void lg_col_complement_kernel(const unsigned long long* __restrict__ bits,
                                                                unsigned long long* __restrict__ comp,
                                                                unsigned long long* __restrict__ sums, int H, int W, int WW) {
    const int b = blockIdx.y;
    const int per_frame = H * WW;
    const unsigned long long* fb = bits + (size_t)b * per_frame;
    unsigned long long* fc = comp + (size_t)b * per_frame;
    unsigned long long sx = 0, sy = 0, n = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_frame; i += gridDim.x * 256) {
        const int y = i / WW, w = i - y * WW;
        const unsigned long long fm = lg_frame_word_mask(W, WW, w);
        unsigned long long v = fb[i] & fm;
        fc[i] = ~v & fm;
        if (sums && v) {
            const unsigned long long c = (unsigned long long)__popcll(v);
            n += c;
            sy += c * (unsigned long long)y;
            sx += c * (unsigned long long)(64 * w);
            for (; v; v &= v - 1ull) sx += (unsigned long long)__builtin_ctzll(v);
        }
    }
    if (!sums) return;
    // (every lane of the wave reaches the shuffles: the loop above has no early exit)
    n = lg_wave_sum_u64(n); sx = lg_wave_sum_u64(sx); sy = lg_wave_sum_u64(sy);
    if ((threadIdx.x & 63) == 0 && n) {
        unsigned long long* fs = sums + (size_t)b * LG_COL_SUMS;
        atomicAdd(&fs[0], sx); atomicAdd(&fs[1], sy); atomicAdd(&fs[2], n);
    }
}

struct LgColSe { LgSeSpans se; LgStemPlan plan; };
__global__ __launch_bounds__(256) void lg_col_erode_step_kernel(const unsigned long long* __restrict__ src,
                                                                unsigned long long* __restrict__ dst, const LgWin* __restrict__ win,
                                                                int H, int W, int WW, LgColSe k) {
    const int b = blockIdx.y;
    const int per_frame = H * WW;
    const LgWin wn = win[b];
    const unsigned long long* fs = src + (size_t)b * per_frame;
    unsigned long long* fd = dst + (size_t)b * per_frame;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_frame; i += gridDim.x * 256) {
        const int y = i / WW, w = i - y * WW;
        fd[i] = lg_erode_step_word(fs, H, W, WW, y, w, wn.bx0, wn.bx1, wn.by0, wn.by1, k.se, k.plan);
    }
}

// One thread per pixel of the frame.
__global__ __launch_bounds__(256) void lg_col_unpack_kernel(const unsigned long long* __restrict__ comp, uint8_t* __restrict__ safe, int H,
                                                            int W, int WW) {
    const int b = blockIdx.y;
    const size_t px = (size_t)H * W;
    const unsigned long long* fc = comp + (size_t)b * H * WW;
    uint8_t* fo = safe + (size_t)b * px;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        fo[i] = ((fc[(size_t)y * WW + (x >> 6)] >> (x & 63)) & 1ull) ? 0 : 1;
    }
}

// ============================================================================ tip penalty as written
__global__ __launch_bounds__(256) void lg_col_tip_kernel(const uint8_t* __restrict__ safe, float* __restrict__ out, int H, int W,
                                                         uint32_t init0, uint32_t max_fix) {
    const int b = blockIdx.y;
    const size_t px = (size_t)H * W;
    const uint8_t* fs = safe + (size_t)b * px;
    float* fo = out + (size_t)b * px;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        fo[i] = fs[i] ? lg_tip_value(lg_tip_fix(x, y, H, W, init0), max_fix) : 0.0f;
    }
}

// ============================================================================ fusion + first maximum
// The workgroup's best key and "some value > 0" into the frame's words: one 64-bit atomicMax and at most one atomicOr.
__device__ __forceinline__ void lg_col_reduce(unsigned long long key, bool pos, const LgColReduce& red, int b) {
    __shared__ unsigned long long s_key[4];
    __shared__ int s_pos[4];
    key = lg_wave_max_u64(key);
    const bool any = __ballot(pos) != 0ull;
    const int t = threadIdx.x;
    if ((t & 63) == 0) { s_key[t >> 6] = key; s_pos[t >> 6] = any ? 1 : 0; }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < 4; k++) key = s_key[k] > key ? s_key[k] : key;
        atomicMax(&red.key[b], key);
        if (s_pos[0] | s_pos[1] | s_pos[2] | s_pos[3]) atomicOr(&red.any[b], 1);
    }
}

// trad = float32(w_approach approach + w_sdf sdf + w_flat flatness + w_tip (1 - tip)) (1 - stem) valid, valid = distance >
// min_edge_distance on `safe` (bkp:98-108): the sum in double from the float32 planes, rounded once.  Pixels outside the bounding
// box of `safe` are not read: both outputs are exactly 0 there.  Every pixel of the frame enters the reduction (np.argmax of a
// plane without a positive value is the first pixel that holds the maximum, on the leaf or not).
__global__ __launch_bounds__(256) void lg_col_fuse_kernel(LgFuseArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const size_t px = (size_t)a.H * a.W, fo = (size_t)b * px;
    const LgWin wn = a.win[b];
    unsigned long long key = 0;
    bool pos = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / a.W), x = (int)(i - (size_t)y * a.W);
        float t = 0.0f;
        uint8_t v = 0;
        if (wn.bx1 >= wn.bx0 && x >= wn.bx0 && x <= wn.bx1 && y >= wn.by0 && y <= wn.by1) {
            const size_t o = fo + i;
            const double s = (double)a.w_approach * (double)a.approach[o] + (double)a.w_sdf * (double)a.sdf[o] +
                             (double)a.w_flat * (double)a.flat[o] + (double)a.w_tip * (1.0 - (double)a.tip[o]);
            v = (a.dist[o] > a.min_edge_distance && a.safe[o]) ? 1 : 0;
            t = (float)s * (1.0f - a.stem[o]);
            t = t * (v ? 1.0f : 0.0f);
        }
        a.trad[fo + i] = t;
        a.valid[fo + i] = v;
        const unsigned long long k = lg_argmax_key(t, (uint32_t)i);
        key = k > key ? k : key;
        pos = pos || t > 0.0f;
    }
    lg_col_reduce(key, pos, a.red, b);
}

__global__ __launch_bounds__(256) void lg_col_argmax_kernel(const float* __restrict__ plane, LgColReduce red, int H, int W) {
    const int b = blockIdx.y;
    const size_t px = (size_t)H * W;
    const float* fp = plane + (size_t)b * px;
    unsigned long long key = 0;
    bool pos = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const float t = fp[i];
        const unsigned long long k = lg_argmax_key(t, (uint32_t)i);
        key = k > key ? k : key;
        pos = pos || t > 0.0f;
    }
    lg_col_reduce(key, pos, red, b);
}

// ============================================================================ the pick
// One thread per frame (bkp:111-117): the arg-max where some value is positive, else calculate_centroid of the ORIGINAL mask --
// sum x / n and sum y / n in double from the integer sums, rounded to float32 as the tensor mean is, truncated as int() does.
// An empty original mask has no point (int(nan) raises in the reference, twice: its None triple).
__global__ __launch_bounds__(64) void lg_col_pick_kernel(LgColReduce red, const unsigned long long* __restrict__ sums,
                                                         const float* __restrict__ depth, LgColPick pick, int B, int H, int W) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float mx;
    uint32_t idx;
    lg_argmax_unkey(red.key[b], &mx, &idx);
    const unsigned long long n = sums[(size_t)b * LG_COL_SUMS + 2];
    int found = 0, x = 0, y = 0, by_max = 0;
    if (n > 0) {
        found = 1;
        if (red.any[b]) {
            by_max = 1;
            y = (int)(idx / (uint32_t)W); x = (int)(idx - (uint32_t)y * (uint32_t)W);
        } else {
            x = (int)(float)((double)sums[(size_t)b * LG_COL_SUMS] / (double)n);
            y = (int)(float)((double)sums[(size_t)b * LG_COL_SUMS + 1] / (double)n);
        }
        x = x < 0 ? 0 : x >= W ? W - 1 : x;   // (a mean of coordinates inside the frame lies inside it; the arg-max is a pixel)
        y = y < 0 ? 0 : y >= H ? H - 1 : y;
    }
    pick.n[b] = found;
    pick.xy[2 * b] = x; pick.xy[2 * b + 1] = y;
    pick.info[2 * b] = mx;
    pick.info[2 * b + 1] = found ? depth[(size_t)b * H * W + (size_t)y * W + x] : 0.0f;
    pick.meta[2 * b] = by_max;
    pick.meta[2 * b + 1] = __float_as_int(mx);
}

__global__ __launch_bounds__(64) void lg_col_rows_kernel(LgColPick pick, lg_grasp_result* __restrict__ res, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    res[b].n_candidates = pick.meta[2 * b];
    res[b].ml_used = 0;
    res[b].best_score = __int_as_float(pick.meta[2 * b + 1]);
}

unsigned frame_blocks(long long items) {   // grid-stride loops: enough workgroups to fill the part, no more than the work
    return (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, 1024));
}

}  // namespace

void lg_launch_col_complement(const unsigned long long* bits, unsigned long long* comp, unsigned long long* sums, int B, int H, int W,
                              int WW, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_complement_kernel, dim3(frame_blocks((long long)H * WW), B), dim3(256), 0, s, bits, comp, sums, H, W, WW);
}

void lg_launch_col_erode_step(const unsigned long long* src, unsigned long long* dst, const LgWin* win, int B, int H, int W, int WW, int k,
                              hipStream_t s) {
    LgColSe se;
    lg_make_se_spans(k, &se.se);
    lg_make_stem_plan(se.se, &se.plan);
    hipLaunchKernelGGL(lg_col_erode_step_kernel, dim3(frame_blocks((long long)H * WW), B), dim3(256), 0, s, src, dst, win, H, W, WW, se);
}

void lg_launch_col_unpack(const unsigned long long* comp, uint8_t* safe, int B, int H, int W, int WW, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_unpack_kernel, dim3(frame_blocks((long long)H * W), B), dim3(256), 0, s, comp, safe, H, W, WW);
}

void lg_launch_col_tip(const uint8_t* safe, float* out, int B, int H, int W, uint32_t init0, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_tip_kernel, dim3(frame_blocks((long long)H * W), B), dim3(256), 0, s, safe, out, H, W, init0,
                       lg_tip_fix_max(H, W, init0));
}

void lg_launch_col_fuse(const LgFuseArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_fuse_kernel, dim3(frame_blocks((long long)a.H * a.W), a.B), dim3(256), 0, s, a);
}

void lg_launch_col_argmax(const float* plane, const LgColReduce& red, int B, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_argmax_kernel, dim3(frame_blocks((long long)H * W), B), dim3(256), 0, s, plane, red, H, W);
}

void lg_launch_col_pick(const LgColReduce& red, const unsigned long long* sums, const float* depth, const LgColPick& pick, int B, int H,
                        int W, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_pick_kernel, dim3((B + 63) / 64), dim3(64), 0, s, red, sums, depth, pick, B, H, W);
}

void lg_launch_col_rows(const LgColPick& pick, lg_grasp_result* res, int B, hipStream_t s) {
    hipLaunchKernelGGL(lg_col_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, s, pick, res, B);
}
