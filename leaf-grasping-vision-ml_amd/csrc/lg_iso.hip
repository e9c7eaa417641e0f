// gfx950 kernels of the label-aware isolation map (lg_params.label_aware = 1; include/leafgrasp.h):
// bit rows of the other leaves, their dilation by the 30 and 40 ellipses over the whole frame, the 3x3 chamfer transform of
// each complement by two raster sweeps, and the plane on the pixels of the current leaf.  Reference semantics:
// scripts/utils/grasp_point_selector.py:595-633 with `other_leaves` taken from the label image.  Nothing here runs while the
// mode is off.
#include "lg_iso.h"
#include "lg_bits.h"
#include "lg_wave.h"

#include <algorithm>

// ============================================================================ others' bit rows, any width
// others[b][y][w] bit j = labels[b][y][64 w + j] > 0 && != ids[b]: one wave ballot per word (the launcher of the label pack
// pass takes this when W % 16 != 0; else its own kernel emits the rows in the same read of the labels).
__global__ __launch_bounds__(256) void lg_pack_others_kernel(const int16_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                             unsigned long long* __restrict__ others, uint32_t* __restrict__ iso_mf,
                                                             int H, int W, int WW) {
    const int lane = threadIdx.x & 63, frame = blockIdx.y;
    const int nwords = H * WW;
    const int16_t* fl = labels + (size_t)frame * H * W;
    unsigned long long* fo = others + (size_t)frame * nwords;
    const int id = ids[frame];
    unsigned long long any = 0;
    const int stride = (gridDim.x * 256) >> 6;
    for (int wid = (blockIdx.x * 256 + threadIdx.x) >> 6; wid < nwords; wid += stride) {   // one 64-bit word per wave
        const int row = wid / WW, w = wid - row * WW;
        const int x = w * 64 + lane;
        const int l = (x < W) ? (int)fl[(size_t)row * W + x] : 0;
        const unsigned long long b = __ballot(l > 0 && l != id);
        if (lane == 0) fo[wid] = b;
        any |= b;
    }
    if (any != 0ull && lane == 0) atomicOr(&iso_mf[(size_t)frame * LG_ISO_MF + 2], 1u);
}

void lg_launch_pack_others(const int16_t* labels, const int32_t* ids_dev, unsigned long long* others, uint32_t* iso_mf, int B, int H,
                           int W, int WW, hipStream_t s) {
    const long long full = ((long long)H * WW * 64 + 255) / 256;
    const unsigned nblk = (unsigned)std::max<long long>(1, std::min<long long>(full, 8192 / B));
    hipLaunchKernelGGL(lg_pack_others_kernel, dim3(nblk, B), dim3(256), 0, s, labels, ids_dev, others, iso_mf, H, W, WW);
}

// ============================================================================ whole-frame dilation on bit rows
// One thread per word of a frame, blockIdx.z = the structuring element (0: ellipse 30, 1: ellipse 40): lg_frame_dilate_word, the
// stem chains with the whole frame as their source.  A word whose 192-bit neighbourhood holds no bit costs its loads only (the
// chain's dilations return at once on a zero accumulator); a frame without another leaf is left alone.
struct LgIsoSe { LgSeSpans se[2]; LgStemPlan plan[2]; };
__global__ __launch_bounds__(256) void lg_iso_dilate_kernel(const unsigned long long* __restrict__ others,
                                                            unsigned long long* __restrict__ dil,
                                                            const uint32_t* __restrict__ iso_mf, int B, int H, int W, int WW, LgIsoSe k) {
    const int b = blockIdx.y, f = blockIdx.z;
    if (iso_mf[(size_t)b * LG_ISO_MF + 2] == 0u) return;
    const size_t per_frame = (size_t)H * WW;
    const unsigned long long* fb = others + (size_t)b * per_frame;
    unsigned long long* fd = dil + ((size_t)f * B + b) * per_frame;
    const LgSeSpans& se = k.se[f];
    const LgStemPlan& pl = k.plan[f];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (int)per_frame; i += gridDim.x * 256) {
        const int y = i / WW, w = i - y * WW;
        fd[i] = lg_frame_dilate_word(fb, H, W, WW, y, w, se, pl);
    }
}

void lg_launch_iso_dilate(const unsigned long long* others, unsigned long long* dil, const uint32_t* iso_mf, int B, int H, int W, int WW,
                          hipStream_t s) {
    LgIsoSe k;
    lg_make_se_spans(30, &k.se[0]);
    lg_make_se_spans(40, &k.se[1]);
    lg_make_stem_plan(k.se[0], &k.plan[0]);
    lg_make_stem_plan(k.se[1], &k.plan[1]);
    const long long per_frame = (long long)H * WW;
    const unsigned nblk = (unsigned)std::max<long long>(1, std::min<long long>((per_frame + 255) / 256, 128));
    hipLaunchKernelGGL(lg_iso_dilate_kernel, dim3(nblk, B, 2), dim3(256), 0, s, others, dil, iso_mf, B, H, W, WW, k);
}

// ============================================================================ chamfer 3x3 distance transform
// cv2.distanceTransform(1 - dil, DIST_L2, 3): OpenCV's two raster passes, row after row, in its 16.16 integers with its border
// cells (init0 above, left and right of the frame).  One workgroup of 256 threads per (field, frame), E consecutive columns per
// thread.  A row's recurrence tmp[j] = min(u[j], tmp[j - 1] + a) is a min-plus prefix scan: thread-local chain, then an
// inclusive prefix minimum of key = last value + a * (columns to the right of it) over the wave and over the four waves
// through LDS; the keys stay below 2^32 for every allowed init0 and shape (INT_MAX + 16384 a + 8192 a).  The previous row lives
// in LDS, double buffered.  The backward pass is the same code on the image turned by 180 degrees; its `t0 > a` guard only
// skips updates that cannot lower the value.  Integer minima in any order give OpenCV's integers.
__device__ __forceinline__ uint32_t lg_wave_prefix_min_u32(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v = u < v ? u : v;
    }
    return v;
}

template <int E, bool BWD>
__global__ __launch_bounds__(256) void lg_iso_sweep_kernel(const unsigned long long* __restrict__ dil, uint32_t* __restrict__ fields,
                                                           uint32_t* __restrict__ iso_mf, int B, int H, int W, int WW, uint32_t init0) {
    constexpr int WL = 256 * E;                    // logical columns of the workgroup (>= W)
    __shared__ uint32_t s_row[2][WL + 2];          // a row's final values at [1 + j]; [0] and every j >= W: the border cell
    __shared__ uint32_t s_tot[2][4];
    const int f = blockIdx.x, b = blockIdx.y;
    if (iso_mf[(size_t)b * LG_ISO_MF + 2] == 0u) return;   // (whole workgroup, before any barrier)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c0 = t * E;
    const unsigned long long* fd = dil + ((size_t)f * B + b) * (size_t)H * WW;
    uint32_t* tp = fields + ((size_t)b * 2 + f) * (size_t)H * W;
    for (int i = t; i < 2 * (WL + 2); i += 256) (&s_row[0][0])[i] = init0;
    __syncthreads();
    uint32_t mx = 0;
    // the row's inputs, one row ahead: forward the E source bits, backward the E forward values
    uint32_t in[E];
    auto load_row = [&](int r) {
        if (r >= H) return;
        if (!BWD) {
            // logical = physical; E divides 64 and c0 % E == 0: the E bits lie in one word
            const int w = c0 >> 6;
            const unsigned long long word = (w < WW) ? fd[(size_t)r * WW + w] : 0ull;
            in[0] = (uint32_t)((word >> (c0 & 63)) & (E == 32 ? 0xFFFFFFFFull : ((1ull << E) - 1ull)));
        } else {
            const uint32_t* row = tp + (size_t)(H - 1 - r) * W;
#pragma unroll
            for (int k = 0; k < E; k++) in[k] = (c0 + k < W) ? row[W - 1 - (c0 + k)] : init0;
        }
    };
    load_row(0);
    for (int r = 0; r < H; r++) {
        const int par = r & 1;
        uint32_t v[E];
        {
            const uint32_t* pr = &s_row[par][0];   // previous row: logical column j at [1 + j]
            uint32_t left = pr[c0], mid = pr[c0 + 1];
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint32_t right = pr[c0 + k + 2];
                uint32_t init;
                if (!BWD) init = ((in[0] >> k) & 1u) ? 0u : 0xFFFFFFFFu;   // a set bit of dil = a zero pixel of 1 - dil
                else init = in[k];
                const uint32_t d = (left < right ? left : right) + LG_B3;
                const uint32_t a = mid + LG_A3;
                uint32_t m = d < a ? d : a;
                v[k] = m < init ? m : init;
                left = mid; mid = right;
            }
        }
        load_row(r + 1);   // (in[] of this row has been consumed)
        // ---- same-row chain: thread-local, then across the workgroup
#pragma unroll
        for (int k = 1; k < E; k++) { const uint32_t c = v[k - 1] + LG_A3; v[k] = c < v[k] ? c : v[k]; }
        const uint32_t key = v[E - 1] + (uint32_t)(WL - 1 - (c0 + E - 1)) * LG_A3;
        const uint32_t pin = lg_wave_prefix_min_u32(key, lane);
        uint32_t excl = __shfl_up(pin, 1, 64);
        if (lane == 0) excl = 0xFFFFFFFFu;
        if (lane == 63) s_tot[par][wave] = pin;
        lg_lds_barrier();
#pragma unroll
        for (int w = 0; w < 3; w++) {
            const uint32_t tw = s_tot[par][w];
            if (w < wave) excl = tw < excl ? tw : excl;
        }
        // the value of logical column c0 - 1 (the border cell left of the frame for thread 0)
        const uint32_t cin = (t == 0) ? init0 : excl - (uint32_t)(WL - 1 - (c0 - 1)) * LG_A3;
#pragma unroll
        for (int k = 0; k < E; k++) { const uint32_t c = cin + (uint32_t)(k + 1) * LG_A3; v[k] = c < v[k] ? c : v[k]; }
        // ---- write back: the next row's "previous row" (columns past W stay border cells) and the field
        uint32_t* nr = &s_row[par ^ 1][0];
        const int prow = BWD ? H - 1 - r : r;
#pragma unroll
        for (int k = 0; k < E; k++) {
            const int j = c0 + k;
            nr[1 + j] = (j < W) ? v[k] : init0;
            if (j < W) {
                tp[(size_t)prow * W + (BWD ? W - 1 - j : j)] = v[k];
                if (BWD) mx = v[k] > mx ? v[k] : mx;
            }
        }
        lg_lds_barrier();
    }
    if (BWD) {
        mx = lg_wave_max_u32(mx);
        if (lane == 0) atomicMax(&iso_mf[(size_t)b * LG_ISO_MF + f], mx);
    }
}

int lg_launch_iso_sweeps(const unsigned long long* dil, uint32_t* fields, uint32_t* iso_mf, int B, int H, int W, int WW, uint32_t init0,
                         hipStream_t s) {
    const dim3 grid(2, B), block(256);
    if (W <= 2048) {
        hipLaunchKernelGGL((lg_iso_sweep_kernel<8, false>), grid, block, 0, s, dil, fields, iso_mf, B, H, W, WW, init0);
        hipLaunchKernelGGL((lg_iso_sweep_kernel<8, true>), grid, block, 0, s, dil, fields, iso_mf, B, H, W, WW, init0);
    } else if (W <= 8192) {
        hipLaunchKernelGGL((lg_iso_sweep_kernel<32, false>), grid, block, 0, s, dil, fields, iso_mf, B, H, W, WW, init0);
        hipLaunchKernelGGL((lg_iso_sweep_kernel<32, true>), grid, block, 0, s, dil, fields, iso_mf, B, H, W, WW, init0);
    } else {
        return -1;
    }
    return 0;
}

// ============================================================================ the plane on the current leaf (dense calls)
// After lg_final_kernel on the same stream: isolation of the pixels of the current leaf inside its bounding box, from the two
// transforms.  Every other pixel of the plane is 0 in both modes (the plane is multiplied by the current leaf's mask).
__global__ __launch_bounds__(256) void lg_iso_plane_kernel(LgIsoFields fl, const unsigned long long* __restrict__ bits,
                                                           const LgWin* __restrict__ win, float* __restrict__ iso, int H, int W, int WW,
                                                           float w_close, float w_wide, float ramp_top, float ramp_step) {
    const int b = blockIdx.y;
    const uint32_t* imf = fl.iso_mf + (size_t)b * LG_ISO_MF;
    if (imf[2] == 0u) return;
    const LgWin w = win[b];
    if (w.bx1 < w.bx0 || w.by1 < w.by0) return;
    const int bw = w.bx1 - w.bx0 + 1, n = bw * (w.by1 - w.by0 + 1);
    const uint32_t maxc = imf[0], maxw = imf[1];
    const uint32_t* fc = fl.fields + (size_t)b * 2 * H * W;
    const unsigned long long* fb = bits + (size_t)b * H * WW;
    float* out = iso + (size_t)b * H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ry = i / bw, y = w.by0 + ry, x = w.bx0 + (i - ry * bw);
        if (!((fb[(size_t)y * WW + (x >> 6)] >> (x & 63)) & 1ull)) continue;
        const size_t o = (size_t)y * W + x;
        const float ramp = __builtin_fmaf(ramp_step, (float)y, ramp_top);
        out[o] = lg_iso_value(fc[o], fc[(size_t)H * W + o], maxc, maxw, w_close, w_wide, ramp);
    }
}

void lg_launch_iso_plane(const LgIsoFields& f, const unsigned long long* bits, const LgWin* win, float* iso, int B, int H, int W, int WW,
                         float w_close, float w_wide, float ramp_top, float ramp_step, hipStream_t s) {
    const long long px = (long long)H * W;
    const unsigned nblk = (unsigned)std::max<long long>(1, std::min<long long>((px + 255) / 256, 256));
    hipLaunchKernelGGL(lg_iso_plane_kernel, dim3(nblk, B), dim3(256), 0, s, f, bits, win, iso, H, W, WW, w_close, w_wide, ramp_top,
                       ramp_step);
}
