// 32 x 32 windows around points: the CNN's 9-channel patch gather (with the deferred planes), training-sample harvesting and
// the negative-sample masks.  Reference semantics: scripts/utils/grasp_point_selector.py, ml_grasp_optimizer/data_collector.py.
#include "lg_patches.h"
#include "lg_bits.h"
#include "lg_iso.h"
#include "lg_pixel.h"
#include "lg_planes.h"

#include <type_traits>

// ============================================================================ 9-channel patch gather
// get_ml_score feature assembly (grasp_point_selector.py:59-127): 32x32 window [y-16,y+16) x [x-16,x+16),
// replicate-padded (:392-445); channel 0 depth and channels 2..8 (sdf, approach, flatness, isolation,
// distance, accessibility, stem) are min-max normalised per patch when max > min; channel 1 = raw mask.
struct LgGatherMaps { const float* p[7]; };
// HALO: write the interior of the first 9 of the 12 haloed planes [12][34][36] (pixel (y,x) at [y+1][x+1]; the CNN's staging layout, lg_cnn.hip;
// the halo itself is zeroed once when the workspace is allocated) instead of dense [9][32][32].
// tile_state (sparse planes): on a tile with state 0 the seven planes were not written; its pixels take the constant tile's
// values (flatness lg_const_flat(flat_scale), every other plane 0 -- distance too: the sweeps write 0 at a pixel off the leaf,
// and the final kernel's constant path writes 0 outside their window), so the patches are those of the written planes.
// DEFER (deferred planes; fa = the arguments of the score-only plane launch over these frames): sdf, approach, isolation,
// accessibility and stem were not stored.  A window's distinct pixels form one rectangle of at most 32 x 32 (replicate clamping
// only repeats its border pixels); every pixel of it on a state-1 tile goes through lg_pixels4, four pixels of a row per
// thread as in the plane kernel, with the stored flatness and distance, behind the plane kernel's own wave-level predicate
// (lg_wave_on_mask: the sign of a zero depends on it).  The window then reads those five planes from LDS.
struct LgGatherNoDefer { int unused; };
// numpy's min and max return NaN for a window that holds one (fminf / fmaxf skip it)
__device__ __forceinline__ float lg_nanmin(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float lg_nanmax(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// LA (label-aware mode, with DEFER; false: the extra argument is an unused placeholder): isolation of a frame that has another
// leaf comes from the two chamfer-3 transforms (lg_iso_value) instead of the plane kernel's closed form.
template <bool HALO, bool DEFER, bool LA = false>
__global__ __launch_bounds__(256) void lg_gather_kernel(const float* __restrict__ depth,
                                                        const uint8_t* __restrict__ mask, LgGatherMaps maps,
                                                        const uint8_t* __restrict__ tile_state, float flat_scale, int H,
                                                        int W, int k, const int32_t* __restrict__ xy,
                                                        const int32_t* __restrict__ n, float* __restrict__ patches,
                                                        const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                        typename std::conditional<DEFER, LgFinalArgs, LgGatherNoDefer>::type fa,
                                                        typename std::conditional<LA, LgIsoFields, LgGatherNoDefer>::type iso) {
    __shared__ float s_pl[DEFER ? 5 : 1][DEFER ? 1024 : 1];   // sdf, approach, isolation, accessibility, stem of the rectangle
    __shared__ float s_mn[4], s_mx[4];
    __shared__ int s_mat[3][2];   // state of the <= 3 x 2 tiles under the window (rows ty_lo.., columns tx_lo..)
    constexpr int PL = HALO ? 34 * 36 : 1024, RP = HALO ? 36 : 32, O0 = HALO ? 37 : 0;
    int ci = blockIdx.x, frame = blockIdx.y;
    const int t = threadIdx.x;
    const int j = frame * k + ci;   // patch slot
    if (list) {                     // survivors only: slot j takes list entry j (a candidate below n[frame]), the rest is left alone
        if (j >= *count) return;
        const int e = list[j];
        frame = e / k;
        ci = e - frame * k;
    }
    float* outp = patches + (size_t)j * (HALO ? 12 : 9) * PL + O0;   // haloed patches carry 3 more (zero) planes
    if (ci >= n[frame]) {
        for (int c = 0; c < 9; c++)
            for (int i = t; i < 1024; i += 256) outp[c * PL + (i >> 5) * RP + (i & 31)] = 0.0f;
        return;
    }
    const int px = xy[((size_t)frame * k + ci) * 2], py = xy[((size_t)frame * k + ci) * 2 + 1];
    const size_t fo = (size_t)frame * H * W;
    // the clamped window spans rows clamp(py-16) .. clamp(py+15) (32 rows: at most 3 tile rows) and 32 columns (at most 2)
    const int ty_lo = min(max(py - 16, 0), H - 1) / LG_TH, tx_lo = min(max(px - 16, 0), W - 1) / LG_TW;
    if (t < 6) {
        const int tiles_x = (W + LG_TW - 1) / LG_TW, tiles_y = (H + LG_TH - 1) / LG_TH;
        const int ty = ty_lo + t / 2, tx = tx_lo + t % 2;
        s_mat[t / 2][t % 2] = (!tile_state || ty >= tiles_y || tx >= tiles_x) ? 1
                              : tile_state[(size_t)frame * tiles_x * tiles_y + ty * tiles_x + tx];
    }
    __syncthreads();
    bool mat[4];
    size_t o_[4];
    int li_[4];   // (deferred planes) the pixel's place in the rectangle
    const int ry0 = max(py - 16, 0), rx0 = max(px - 16, 0);   // first row and column of the window's rectangle
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int i = t + 256 * q;
        int yy = py - 16 + (i >> 5), xx = px - 16 + (i & 31);
        yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
        xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
        o_[q] = fo + (size_t)yy * W + xx;
        li_[q] = (yy - ry0) * 32 + (xx - rx0);
        mat[q] = s_mat[yy / LG_TH - ty_lo][xx / LG_TW - tx_lo] != 0;
    }
    const float flat1 = lg_const_flat(flat_scale);
    if constexpr (DEFER) {
        const int RH = min(py + 15, H - 1) - ry0 + 1, RW = min(px + 15, W - 1) - rx0 + 1;
        const int WW = fa.WW;
        const unsigned long long* bits = fa.bits + (size_t)frame * H * WW;
        const unsigned long long* stemb = fa.stem_bits + (size_t)frame * H * WW;
        // four pixels of a rectangle row per thread (columns past the rectangle or the frame store nothing)
        const int ry = t >> 3, gx = 4 * (t & 7);
        if (ry < RH && gx < RW) {
            const int y = ry0 + ry, x0 = rx0 + gx;
            float o_flat[4];
            unsigned mnib = 0, snib = 0, on = 0, live = 0;   // per pixel: mask bit, stem bit, its wave of the plane kernel held a leaf pixel, state-1 tile
            float din[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = min(x0 + j, W - 1);
                const size_t wi = (size_t)y * WW + (x >> 6);
                mnib |= (unsigned)((bits[wi] >> (x & 63)) & 1ull) << j;
                snib |= (unsigned)((stemb[wi] >> (x & 63)) & 1ull) << j;
                // (on a state-0 tile the distance plane holds stale or unwritten data in sparse mode: whatever is computed from
                // it is dropped below, where `live` picks the constant tile's values)
                din[j] = maps.p[LG_MAP_DISTANCE][fo + (size_t)y * W + x];
                o_flat[j] = 0.0f;   // flatness enters `traditional` only, which the gather does not use: no load
                if ((fa.no_skip & 2) || lg_wave_on_mask(bits, H, WW, y, x >> 6)) on |= 1u << j;
                if (s_mat[y / LG_TH - ty_lo][x / LG_TW - tx_lo] != 0) live |= 1u << j;
            }
            float o_sdf[4], o_app[4], o_iso[4], o_acc[4], o_stem[4], o_trad[4];
            bool o_valid[4];
            const LgPixFrame pf = lg_pix_frame(&fa, fa.fp + frame, fa.maxfix + LG_MF * (size_t)frame);
            lg_pixels4<true>(&fa, pf, y, x0, H, W, mnib, snib, din, o_flat, fa.w_flat, o_sdf, o_app, o_iso, o_acc, o_stem, o_trad, o_valid);
            if constexpr (LA) {
                const uint32_t* imf = iso.iso_mf + (size_t)frame * LG_ISO_MF;
                if (imf[2] != 0u) {
                    const uint32_t* fc = iso.fields + (size_t)frame * 2 * H * W;
                    const float ramp = __builtin_fmaf(fa.iso_ramp_step, (float)y, fa.iso_ramp_top);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const size_t o = (size_t)y * W + min(x0 + j, W - 1);
                        o_iso[j] = lg_iso_value(fc[o], fc[(size_t)H * W + o], imf[0], imf[1], fa.iso_w_close, fa.iso_w_wide, ramp) *
                                   (((mnib >> j) & 1u) ? 1.0f : 0.0f);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gx + j < RW) {
                    const bool lv = (live >> j) & 1u, w_on = (on >> j) & 1u;   // off a state-1 tile: the constant tile's values
                    const int li = ry * 32 + gx + j;
                    s_pl[0][li] = lv && w_on ? o_sdf[j] : 0.0f;
                    s_pl[1][li] = lv && w_on ? o_app[j] : 0.0f;
                    s_pl[2][li] = lv && w_on ? o_iso[j] : 0.0f;
                    s_pl[3][li] = lv && w_on ? o_acc[j] : 0.0f;
                    s_pl[4][li] = lv && w_on ? o_stem[j] : 0.0f;
                }
        }
        __syncthreads();
    }
    for (int c = 0; c < 9; c++) {
        float v[4];
        float mn = INFINITY, mx = -INFINITY;
        const float cst = (c == 2 + LG_MAP_FLATNESS) ? flat1 : 0.0f;   // the constant tile's value of plane c - 2
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const size_t o = o_[q];
            float val;
            if (DEFER && c >= 2 && c != 2 + LG_MAP_DISTANCE && c != 2 + LG_MAP_FLATNESS)   // sdf, approach | isolation | accessibility, stem
                val = s_pl[c - 2 < LG_MAP_FLATNESS ? c - 2 : c - 2 < LG_MAP_DISTANCE ? c - 3 : c - 4][li_[q]];
            else
                val = (c == 0) ? depth[o] : (c == 1) ? (mask[o] ? 1.0f : 0.0f) : mat[q] ? maps.p[c - 2][o] : cst;
            v[q] = val;
            mn = lg_nanmin(mn, val);
            mx = lg_nanmax(mx, val);
        }
        if (c != 1) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                mn = lg_nanmin(mn, __shfl_xor(mn, o, 64));
                mx = lg_nanmax(mx, __shfl_xor(mx, o, 64));
            }
            __syncthreads();  // previous channel's readers are done
            if ((t & 63) == 0) { s_mn[t >> 6] = mn; s_mx[t >> 6] = mx; }
            __syncthreads();
            mn = lg_nanmin(lg_nanmin(s_mn[0], s_mn[1]), lg_nanmin(s_mn[2], s_mn[3]));
            mx = lg_nanmax(lg_nanmax(s_mx[0], s_mx[1]), lg_nanmax(s_mx[2], s_mx[3]));
            if (mx > mn) {   // false with a NaN in the channel, as numpy's p.max() > p.min(): the channel stays raw
                const float range = mx - mn;
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = (v[q] - mn) / range;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = t + 256 * q;
            outp[c * PL + (i >> 5) * RP + (i & 31)] = v[q];
        }
        if (HALO && t < 200) {
            // the plane's 200 halo floats, zero as they already are: a cache line the kernel writes only in part leaves
            // the L2 as a masked write (tools/ubench/partial_lines.hip)
            float* pl = outp + c * PL - O0;
            const int hi = t < 72 ? (t < 36 ? t : 33 * 36 + (t - 36))              // top and bottom rows
                                  : (t < 104 ? (t - 72 + 1) * 36                     // left column of rows 1..32
                                             : ((t - 104) / 3 + 1) * 36 + 33 + (t - 104) % 3);   // columns 33..35
            pl[hi] = 0.0f;
        }
    }
}

void lg_launch_gather(const float* depth, const uint8_t* mask, const float* const* maps_host, const uint8_t* tile_state,
                      float flat_scale, int B, int H, int W, int k, const int32_t* xy, const int32_t* n, float* patches,
                      bool haloed, hipStream_t s, const int32_t* list, const int32_t* count, const LgFinalArgs* defer,
                      const LgIsoFields* iso) {
    LgGatherMaps gm;
    for (int i = 0; i < 7; i++) gm.p[i] = maps_host[i];
    const LgGatherNoDefer nd = {0};
    if (defer && iso)   // (label-aware mode: isolation from the transforms; without `defer` the gather reads the stored plane)
        hipLaunchKernelGGL((lg_gather_kernel<true, true, true>), dim3(k, B), dim3(256), 0, s, depth, mask, gm, tile_state, flat_scale, H,
                           W, k, xy, n, patches, list, count, *defer, *iso);
    else if (defer)   // (lg_select_grasp*: haloed patches; the frames and their tile_state are those of *defer)
        hipLaunchKernelGGL((lg_gather_kernel<true, true>), dim3(k, B), dim3(256), 0, s, depth, mask, gm, tile_state, flat_scale, H, W, k,
                           xy, n, patches, list, count, *defer, nd);
    else if (haloed)
        hipLaunchKernelGGL((lg_gather_kernel<true, false>), dim3(k, B), dim3(256), 0, s, depth, mask, gm, tile_state, flat_scale, H, W, k,
                           xy, n, patches, list, count, nd, nd);
    else
        hipLaunchKernelGGL((lg_gather_kernel<false, false>), dim3(k, B), dim3(256), 0, s, depth, mask, gm, tile_state, flat_scale, H, W,
                           k, xy, n, patches, list, count, nd, nd);
}

// ============================================================================ training-sample harvesting
// EnhancedGraspDataCollector (scripts/utils/ml_grasp_optimizer/data_collector.py): raw, un-normalised 32x32 windows
// [y-16, y+16) x [x-16, x+16) of depth, mask and the seven score planes around n points of ONE frame
// (_extract_patches :91-173), optionally rotated by rot[i] quarter turns like torch.rot90(t, k, dims=(-2,-1))
// (_generate_augmented_samples :250-293).  flags[i]: bit 0 non-finite depth, bit 1 empty mask patch, bit 2 non-finite
// score value, bit 3 window not inside the frame (nothing is written for that point).
__global__ __launch_bounds__(256) void lg_harvest_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                         LgGatherMaps maps, int H, int W, const int32_t* __restrict__ xy,
                                                         const int32_t* __restrict__ rot, float* __restrict__ out_depth,
                                                         float* __restrict__ out_mask, float* __restrict__ out_scores,
                                                         int32_t* __restrict__ flags) {
    __shared__ int s_flag, s_any;
    const int i = blockIdx.x, t = threadIdx.x;
    const int px = xy[2 * i], py = xy[2 * i + 1];
    const int k = rot ? (rot[i] & 3) : 0;
    if (t == 0) { s_flag = 0; s_any = 0; }
    __syncthreads();
    // the reference's slices [y-16:y+16, x-16:x+16] (:103-104) are full for 16 <= x <= W-16, 16 <= y <= H-16: the far
    // edge is inclusive, unlike _check_boundaries :83-89, which collect_sample applies to the positive point only.
    // (compared as px > W - 16: px + 16 would wrap for a coordinate near INT_MAX and let the window through)
    if (px < 16 || py < 16 || px > W - 16 || py > H - 16) {
        if (t == 0) flags[i] = 8;
        return;
    }
    int fl = 0, any = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int o = t + 256 * q, r = o >> 5, c = o & 31;
        // torch.rot90: k=1: out[r][c] = in[c][31-r]; k=2: in[31-r][31-c]; k=3: in[31-c][r]
        const int sr = k == 0 ? r : k == 1 ? c : k == 2 ? 31 - r : 31 - c;
        const int sc = k == 0 ? c : k == 1 ? 31 - r : k == 2 ? 31 - c : r;
        const size_t src = (size_t)(py - 16 + sr) * W + (px - 16 + sc);
        const float d = depth[src];
        const float m = mask[src] ? 1.0f : 0.0f;
        if (!isfinite(d)) fl |= 1;
        any |= (m != 0.0f);
        out_depth[(size_t)i * 1024 + o] = d;
        out_mask[(size_t)i * 1024 + o] = m;
#pragma unroll
        for (int ch = 0; ch < 7; ch++) {
            const float v = maps.p[ch][src];
            if (!isfinite(v)) fl |= 4;
            out_scores[((size_t)i * 7 + ch) * 1024 + o] = v;
        }
    }
    if (fl) atomicOr(&s_flag, fl);
    if (any) atomicOr(&s_any, 1);
    __syncthreads();
    if (t == 0) flags[i] = s_flag | (s_any ? 0 : 2);
}

void lg_launch_harvest(const float* depth, const uint8_t* mask, const float* const* maps_host, int H, int W, int n,
                       const int32_t* xy, const int32_t* rot, float* out_depth, float* out_mask, float* out_scores,
                       int32_t* flags, hipStream_t s) {
    LgGatherMaps gm;
    for (int i = 0; i < 7; i++) gm.p[i] = maps_host[i];
    hipLaunchKernelGGL(lg_harvest_kernel, dim3(n), dim3(256), 0, s, depth, mask, gm, H, W, xy, rot, out_depth, out_mask,
                       out_scores, flags);
}

// Negative-sample regions (data_collector.py:426-466):
//   tip  = (cv2.dilate(dist, ones(5,5)) == dist) & mask      local maxima of the distance transform (:430-437)
//   stem = erode(erode(mask with rows < int(0.75 H) cleared, ellipse 5x5), ellipse 5x5)  (:449-456), iteration `pass`
// cv2's morphology border is "ignore": a dilation never sees values outside the frame, an erosion is not eroded by it.
__global__ __launch_bounds__(256) void lg_tip_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ mask,
                                                     uint8_t* __restrict__ tip, int H, int W) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float d = dist[(size_t)y * W + x];
    float mx = d;
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int xx = x + dx;
            if (xx >= 0 && xx < W) mx = fmaxf(mx, dist[(size_t)yy * W + xx]);
        }
    }
    tip[(size_t)y * W + x] = (mx == d && mask[(size_t)y * W + x]) ? 1 : 0;
}
__global__ __launch_bounds__(256) void lg_erode5_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H,
                                                        int W, int first_row) {
    // 5x5 MORPH_ELLIPSE: rows -2 / +2 hold the centre column only, rows -1..1 all five columns; rows < first_row of src
    // count as background (stem_region[:int(0.75*height)] = 0)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    bool keep = true;
    for (int dy = -2; dy <= 2 && keep; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        const int r = (dy == -2 || dy == 2) ? 0 : 2;
        for (int dx = -r; dx <= r; dx++) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            if (yy < first_row || !src[(size_t)yy * W + xx]) { keep = false; break; }
        }
    }
    dst[(size_t)y * W + x] = keep ? 1 : 0;
}

void lg_launch_negative_masks(const float* dist, const uint8_t* mask, uint8_t* tip, uint8_t* stem, uint8_t* scratch, int H,
                              int W, hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4), block(256);
    hipLaunchKernelGGL(lg_tip_kernel, grid, block, 0, s, dist, mask, tip, H, W);
    const int first_row = (int)(0.75 * (double)H);   // int(0.75 * height)
    hipLaunchKernelGGL(lg_erode5_kernel, grid, block, 0, s, mask, scratch, H, W, first_row);
    hipLaunchKernelGGL(lg_erode5_kernel, grid, block, 0, s, scratch, stem, H, W, 0);
}
