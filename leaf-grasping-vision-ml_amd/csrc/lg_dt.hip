// gfx950 kernels of the distance transform: sweep window, border maxima of d_out, the two raster sweeps, run distances and
// the three forms of the sweep-free row search (lg_dt.h: lg_dt_form).  Reference semantics: cv2.distanceTransform as used by
// scripts/utils/grasp_point_selector.py; design: DESIGN.md, "Distance transform".
#include "lg_dt.h"
#include "lg_wave.h"

#include <limits.h>
#include <algorithm>
#include <type_traits>

// ============================================================================ wave helpers of the distance transform
__device__ __forceinline__ int lg_dpp_row_shr(int old, int v, int n) {
    switch (n) {  // dpp_ctrl must be an immediate
        case 1: return __builtin_amdgcn_update_dpp(old, v, 0x111, 0xf, 0xf, false);
        case 2: return __builtin_amdgcn_update_dpp(old, v, 0x112, 0xf, 0xf, false);
        case 4: return __builtin_amdgcn_update_dpp(old, v, 0x114, 0xf, 0xf, false);
        default: return __builtin_amdgcn_update_dpp(old, v, 0x118, 0xf, 0xf, false);
    }
}
// inclusive prefix-min over the 64 lanes of a wave (DPP row shifts + row broadcasts, gfx9 family)
__device__ __forceinline__ int lg_wave_prefix_min(int v) {
    const int id = INT_MAX;
    v = min(v, lg_dpp_row_shr(id, v, 1));
    v = min(v, lg_dpp_row_shr(id, v, 2));
    v = min(v, lg_dpp_row_shr(id, v, 4));
    v = min(v, lg_dpp_row_shr(id, v, 8));
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1,3
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2,3
    return v;
}
__device__ __forceinline__ int lg_wave_shr1(int old, int v) {  // lane i <- lane i-1 (lane 0 keeps old)
    return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int lg_wave_shl1(int old, int v) {  // lane i <- lane i+1 (lane 63 keeps old)
    return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xf, 0xf, false);
}
// minimum over the wave in six DPP steps (quads, half rows, rows, then the two row broadcasts): every lane gets it
__device__ __forceinline__ uint32_t lg_wave_min_u32(uint32_t v) {
#define LG_DPP_MIN(CTRL, RM) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, RM, 0xf, false))
    LG_DPP_MIN(0xB1, 0xf);    // quad_perm 1 0 3 2
    LG_DPP_MIN(0x4E, 0xf);    // quad_perm 2 3 0 1
    LG_DPP_MIN(0x141, 0xf);   // row_half_mirror
    LG_DPP_MIN(0x140, 0xf);   // row_mirror
    LG_DPP_MIN(0x142, 0xa);   // row_bcast15 into rows 1 and 3
    LG_DPP_MIN(0x143, 0xc);   // row_bcast31 into rows 2 and 3
#undef LG_DPP_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ============================================================================ sweep window (mask bounding box)
// One workgroup, thread = frame (frames t, t + 1024, ...): LgWin of every frame (lg_win_from_box, lg_dt.h) from the bounding
// box and area the bit-row pass left in the frame's maxfix words.
//
// Search or sweeps is decided for the BATCH (search_mode 2): the search's time grows like the sum over the frames of area^1.5
// (pixels x their depth), the sweeps' like the rows of the tallest window whatever the batch (one workgroup per frame, all at
// once) -- and a batch of which one half is searched while the other half is swept takes as long as both together (measured:
// 1.1 ms per 256 benchmark frames against 0.7 either way; the two forms do not run beside each other as their streams suggest).
// The per-frame costs are integers: the workgroup sums them (and takes the tallest box) through LDS, and every thread takes
// the same decision before it writes its frames; if the sweeps win, no frame is searched.
__global__ __launch_bounds__(1024) void lg_window_kernel(const uint32_t* __restrict__ mf, LgWin* __restrict__ wins, int B, int H, int W,
                                                         int wc, int nw_max, int search_mode, float search_budget, int far) {
    __shared__ unsigned long long s_cost;
    __shared__ unsigned s_rows;
    const int t = threadIdx.x;
    bool sweeps = far != 0;   // (lg_dt_far: the whole frame is swept)
    if (search_mode == 2 && !far) {
        if (t == 0) { s_cost = 0; s_rows = 0; }
        __syncthreads();
        unsigned long long cost = 0;
        unsigned rows = 0;
        for (int f = t; f < B; f += 1024) {
            const LgWin w = lg_win_from_box(mf + (size_t)f * LG_MF + LG_BOX_X0, H, W, wc, nw_max, search_mode);
            if (w.search_in) {
                // its work grows like area^1.5 (pixels x their depth) while the sweeps' time is set by the window's rows
                const float a = (float)w.area;
                cost += (unsigned long long)(a * __builtin_sqrtf(a));
                rows = max(rows, (unsigned)(w.by1 - w.by0 + 1));
            }
        }
        if (cost) atomicAdd(&s_cost, cost);
        if (rows) atomicMax(&s_rows, rows);
        __syncthreads();
        sweeps = (float)s_cost > search_budget * (float)s_rows;
    }
    for (int f = t; f < B; f += 1024) {
        LgWin w = lg_win_from_box(mf + (size_t)f * LG_MF + LG_BOX_X0, H, W, wc, nw_max, search_mode);
        if (sweeps) w.search_in = 0;
        if (far) { w.wx0 = 0; w.nw = nw_max; w.wy0 = 0; w.wy1 = H; w.skip_out = 0; }
        wins[f] = w;
    }
}

void lg_launch_window(const uint32_t* mf, LgWin* win, int B, int H, int W, int search_mode, hipStream_t s, uint32_t init0) {
    int nw = 0;
    const int wc = lg_dt_geometry(W, &nw);
    // mode 2: search while sum over the frames of area^1.5 <= LG_SEARCH_BUDGET * rows of the tallest window: 0.69 ms for 256
    // benchmark leaves of 100 k pixels in either form (anchors + bands; sweeps: ~1.6 us per row).
    hipLaunchKernelGGL(lg_window_kernel, dim3(1), dim3(1024), 0, s, mf, win, B, H, W, wc, nw, search_mode, LG_SEARCH_BUDGET,
                       lg_dt_far(H, W, init0) ? 1 : 0);
}

// ============================================================================ max d_out outside the sweep window
// d_out(p) = min over leaf pixels q of the 5x5 chamfer norm N(p - q) (see LgWin).  Outside the window, moving p away
// from the leaf's bounding box along x or y increases |dx| (|dy|) for EVERY leaf pixel, and N is monotone in |dx|, |dy|:
// the maximum over the outside region sits on the frame border, and beyond the bounding box's span at a frame corner.
// grid (4, B): side 0 = top row, 1 = bottom row, 2 = left column, 3 = right column.  For a candidate on the top row
// only the topmost leaf pixel of each column can be the nearest one of that column (same dx, smallest dy), etc.
__global__ __launch_bounds__(256) void lg_dout_border_kernel(const unsigned long long* __restrict__ bits,
                                                             const LgWin* __restrict__ wins, uint32_t* __restrict__ maxfix,
                                                             int H, int W, int WW, int wc) {
    extern __shared__ int s_prof[];   // profile of the leaf seen from this side: distance from the border, -1 = no leaf pixel
    const int side = blockIdx.x, frame = blockIdx.y, t = threadIdx.x;
    const LgWin w = wins[frame];
    if (w.bx1 < w.bx0) return;                       // empty mask: handled by the full-frame sweep
    const int wxr = min(W, w.wx0 + w.nw * wc);
    const bool need = side == 0 ? w.wy0 > 0 : side == 1 ? w.wy1 < H : side == 2 ? w.wx0 > 0 : wxr < W;
    if (!need) return;                               // this border line lies inside the window: the sweep covers it
    const unsigned long long* fb = bits + (size_t)frame * H * WW;
    const bool horiz = side < 2;                     // candidates along x, profile indexed by column
    const int lo = horiz ? w.bx0 : w.by0, hi = horiz ? w.bx1 : w.by1, n = hi - lo + 1;
    __shared__ uint32_t s_red[4];                    // minima of the two ends and of the profile; the running maximum
    if (t == 0) { s_red[0] = 0xFFFFFFFFu; s_red[1] = 0xFFFFFFFFu; s_red[2] = 0x7FFFFFFFu; s_red[3] = 0; }
    if (horiz) {
        // item = (64-column word of the bounding box) x (chunk of its rows): a thread walks its chunk from the border inwards, 8
        // rows per round trip; a column's profile entry is the smallest distance at which any chunk saw its bit (atomicMin)
        for (int i = t; i < n; i += 256) s_prof[i] = 0x7FFFFFFF;
        __syncthreads();
        const int q0 = w.bx0 >> 6, nq = (w.bx1 >> 6) - q0 + 1, rows = w.by1 - w.by0 + 1;
        const int nch = max(1, min(256 / nq, (rows + 7) / 8)), rc = (rows + nch - 1) / nch;
        for (int it = t; it < nq * nch; it += 256) {
            const int q = q0 + it % nq, ra = (it / nq) * rc, rb = min(rows, ra + rc);
            unsigned long long seen = 0;
            for (int r0 = ra; r0 < rb; r0 += 8) {
                unsigned long long v[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int r = min(r0 + j, rb - 1);
                    const int y = side == 0 ? w.by0 + r : w.by1 - r;
                    v[j] = fb[(size_t)y * WW + q];
                }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    unsigned long long nb = v[j] & ~seen;
                    seen |= v[j];
                    const int r = min(r0 + j, rb - 1);
                    const int dist = side == 0 ? w.by0 + r : H - 1 - (w.by1 - r);
                    while (nb) {
                        const int c = 64 * q + __builtin_ctzll(nb);
                        nb &= nb - 1;
                        atomicMin(&s_prof[c - lo], dist);
                    }
                }
            }
        }
        __syncthreads();
        for (int i = t; i < n; i += 256) if (s_prof[i] == 0x7FFFFFFF) s_prof[i] = -1;   // (the entries this thread reads below)
    } else {
        for (int i = t; i < n; i += 256) {
            int d = -1;
            const unsigned long long* row = fb + (size_t)(lo + i) * WW;
            if (side == 2) {
                for (int q = w.bx0 >> 6; q <= w.bx1 >> 6; q++) if (row[q]) { d = 64 * q + __builtin_ctzll(row[q]); break; }
            } else {
                for (int q = w.bx1 >> 6; q >= w.bx0 >> 6; q--) if (row[q]) { d = W - 1 - (64 * q + 63 - __builtin_clzll(row[q])); break; }
            }
            s_prof[i] = d;
        }
        __syncthreads();                                 // (s_red)
    }
    // the two ends of the line in full, and the smallest entry: every thread its share of the profile (the entries it wrote)
    const int len = horiz ? W : H;
    {
        uint32_t m = 0x7FFFFFFFu;
        for (int i = t; i < n; i += 256) { const int d = s_prof[i]; if (d >= 0) m = min(m, (uint32_t)d); }
        const uint32_t e0 = lg_wave_min_u32(lg_border_end_part(s_prof, n, lo, 0, t, 256));
        const uint32_t e1 = lg_wave_min_u32(lg_border_end_part(s_prof, n, lo, len - 1, t, 256));
        m = lg_wave_min_u32(m);
        if ((t & 63) == 0) { atomicMin(&s_red[0], e0); atomicMin(&s_red[1], e1); atomicMin(&s_red[2], m); }
    }
    __syncthreads();
    // span candidates, one per lane and round, against the running maximum (lg_border_cand_min).  s_red[3] shares what the
    // other lanes found: a stale, lower value only prunes less, and a maximum does not depend on the order
    const int m = (int)s_red[2];
    uint32_t best = max(s_red[0], s_red[1]);
    for (int c = t; c < n; c += 256) {
        best = max(best, __hip_atomic_load(&s_red[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        const uint32_t d = lg_border_cand_min(s_prof, n, c, m, best);
        if (d > best) { best = d; atomicMax(&s_red[3], d); }
    }
    best = lg_wave_max_u32(best);
    if ((t & 63) == 0 && best) atomicMax(&maxfix[frame * LG_MF + 1], best);
}

void lg_launch_dout_border(const unsigned long long* bits, const LgWin* win, uint32_t* maxfix, int B, int H, int W, int WW,
                           hipStream_t s) {
    const int wc = lg_dt_geometry(W, nullptr);
    const size_t shm = sizeof(int) * (size_t)max(H, W);
    hipLaunchKernelGGL(lg_dout_border_kernel, dim3(4, B), dim3(256), shm, s, bits, win, maxfix, H, W, WW, wc);
}

// ============================================================================ chamfer 5x5 distance transform
// cv2.distanceTransform(src, DIST_L2, 5)  (grasp_point_selector.py:266, :529-530).
// Row-sequential emulation of the two raster sweeps; each image row is one segmented-free min-plus
// prefix scan across the workgroup (tmp[j] = min(u[j], tmp[j-1]+A)  ==  j*A + prefix-min(u[k]-k*A)).
// All arithmetic is exact 16.16 integers, so any evaluation order gives OpenCV's integers.
// grid = (2, B): blockIdx.x selects d_in (src = mask) or d_out (src = !mask).
// The backward sweep is the same code on the 180-degree-rotated image.
template <int T, int E, bool BWD, bool VEC>
__global__ __launch_bounds__(T) void lg_dt5_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ tmp,
                                                   float* __restrict__ dist_out, uint32_t* __restrict__ maxfix,
                                                   const LgWin* __restrict__ wins, int H, int W, uint32_t init0) {
    constexpr int NW = T / 64;
    constexpr int WC = 64 * E;                 // columns per wave
    constexpr int D = (BWD || E > 4) ? 4 : 8;  // rows per prefetch group (two groups are resident)
    // per row and wave: [0] inclusive wave total, [1..2] lane 0's first two pre-carry values,
    // [3..4] lane 63's last two pre-carry values, [5] lane 63's wave-local exclusive prefix
    __shared__ int s_x[2][NW][8];
    const int which = blockIdx.x;
    const int frame = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool far = BWD && lg_dt_far(H, W, init0);
    // ---- sweep window (see LgWin): waves beyond it leave; s_barrier only counts the surviving waves
    const LgWin win = wins[frame];
    const int nwa = win.nw;
    if (wave >= nwa) return;
    if (which == 1 && win.skip_out) return;   // max d_out lies on the frame border (lg_win_from_box): whole workgroup, before any barrier
    if (which == 0 && win.search_in) return;  // d_in of this frame comes from lg_dtsearch_kernel
    const int wx0 = win.wx0, wxe = wx0 + nwa * WC;   // window columns [wx0, wxe); columns >= W are outside the image
    const int wy0 = win.wy0, HW = win.wy1 - win.wy0; // window rows
    const size_t fo = (size_t)frame * H * W;
    const uint8_t* m = mask + fo;
    uint32_t* tp = tmp + ((size_t)frame * 2 + which) * H * W;
    float* dout = (dist_out && which == 0) ? dist_out + fo : nullptr;  // only d_in is a contract plane
    const int pc0 = BWD ? wxe - (t + 1) * E : wx0 + t * E;  // first physical column of this thread (multiple of E)
    constexpr bool vec_ok = VEC;  // host guarantees W % E == 0 when VEC
    const bool full = vec_ok && (pc0 + E <= W);
    const int c0 = t * E;  // first logical column (0 = first window column in sweep order)
    // value of a cell OUTSIDE the window: for d_in an in-image cell there is off the leaf, i.e. a source (0);
    // for d_out, and outside the image, "no path".
    auto outv = [&](int pc, int prow) -> uint32_t {
        return (which == 0 && pc >= 0 && pc < W && prow >= 0 && prow < H) ? 0u : LG_INF;
    };
    auto phys_col = [&](int j) { return BWD ? wxe - 1 - j : wx0 + j; };          // logical -> physical column
    auto phys_row = [&](int r) { return BWD ? win.wy1 - 1 - r : wy0 + r; };       // logical -> physical row

    uint32_t p1[E + 4], p2[E + 2];   // previous row (columns c0-2 .. c0+E+1) and the one before (c0-1 .. c0+E)
#pragma unroll
    for (int i = 0; i < E + 4; i++) p1[i] = outv(phys_col(c0 - 2 + i), phys_row(-1));
#pragma unroll
    for (int i = 0; i < E + 2; i++) p2[i] = outv(phys_col(c0 - 1 + i), phys_row(-2));
    // the cell left of the window in the current row (a source for d_in when it lies in the image)
    const uint32_t edge_l1 = outv(phys_col(-1), wy0), edge_l2 = outv(phys_col(-2), wy0);
    const uint32_t edge_r0 = outv(phys_col(nwa * WC), wy0), edge_r1 = outv(phys_col(nwa * WC + 1), wy0);

    // raw prefetch registers: forward = E mask bytes (packed in up to 2 dwords), backward = E dwords
    constexpr int RAWN = BWD ? E : (E + 3) / 4;
    uint32_t raw[D][RAWN], nxt[D][RAWN];  // group being consumed / group in flight

    // Branch-free prefetch: addresses are clamped into the image and out-of-image lanes are fixed up by
    // selects, so the compiler keeps the loads in flight (a load inside a divergent branch is waited for
    // with vmcnt(0) at the join, which serialises every image row on HBM latency).
    const int pc0c = full ? pc0 : (vec_ok ? max(0, min(pc0, W - E)) : 0);
    auto load_row = [&](int r, uint32_t* dst) {  // r = logical row
        const int prow = phys_row(min(r, HW - 1));
        if (vec_ok) {   // raw values only; out-of-image lanes are fixed up at the point of use
            if (BWD) {
                const uint32_t* src = tp + (size_t)prow * W + pc0c;
#pragma unroll
                for (int q = 0; q < E / 4; q++) {
                    uint4 v = *reinterpret_cast<const uint4*>(src + 4 * q);
                    dst[4 * q + 0] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
                }
            } else {
                const uint8_t* src = m + (size_t)prow * W + pc0c;
                if (E == 4) {
                    dst[0] = *reinterpret_cast<const uint32_t*>(src);
                } else {
                    uint2 v = *reinterpret_cast<const uint2*>(src);
                    dst[0] = v.x; dst[1] = v.y;
                }
            }
        } else {  // generic width: scalar, still branch-free
            if (BWD) {
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const int pc = min(pc0 + k, W - 1);
                    uint32_t v = tp[(size_t)prow * W + pc];
                    dst[k] = (pc0 + k < W) ? v : LG_INF;
                }
            } else {
#pragma unroll
                for (int q = 0; q < RAWN; q++) dst[q] = 0;
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const int pc = min(pc0 + k, W - 1);
                    uint32_t mb = m[(size_t)prow * W + pc];
                    mb = (pc0 + k < W) ? mb : (which ? 0u : 1u);
                    dst[k >> 2] |= (mb & 0xffu) << (8 * (k & 3));
                }
            }
        }
    };

    uint32_t mx = 0;
#pragma unroll
    for (int d = 0; d < D; d++) load_row(d, raw[d]);

    for (int rb = 0; rb < HW; rb += D) {
        // The whole next group is requested up front, so at the next iteration (where the compiler waits for
        // everything outstanding at the loop head) the youngest load is D rows old, not one.
#pragma unroll
        for (int d = 0; d < D; d++) load_row(rb + D + d, nxt[d]);
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int r = rb + d;
            if (r < HW) {
                const int par = r & 1;
                // ---- per-pixel upper bound ("init"): forward: source ? 0 : +inf ; backward: forward result
                uint32_t init[E];
#pragma unroll
                for (int k = 0; k < E; k++) {
                    if (BWD) {
                        init[k] = (vec_ok && !full) ? LG_INF : raw[d][E - 1 - k];
                    } else {
                        uint32_t mb = (raw[d][k >> 2] >> (8 * (k & 3))) & 0xffu;
                        bool nz = which ? (mb == 0) : (mb != 0);
                        if (vec_ok && !full) nz = true;  // out-of-image columns: ordinary non-source pixels
                        init[k] = nz ? 0xFFFFFFFFu : 0u;
                    }
                }
                // ---- contributions of the two previous rows
                uint32_t v[E];
#pragma unroll
                for (int k = 0; k < E; k++) {
                    // group equal weights before adding them: min(x+w, y+w) == min(x,y)+w (no overflow, values < 2^31)
                    const uint32_t mc = min(min(p2[k], p2[k + 2]), min(p1[k], p1[k + 4])) + LG_C5;
                    const uint32_t mb = min(p1[k + 1], p1[k + 3]) + LG_B5;
                    const uint32_t ma = p1[k + 2] + LG_A5;
                    v[k] = min(min(mc, mb), min(ma, init[k]));
                }
                // ---- same-row chain: thread-local, then across the workgroup.  The cell left of the window enters through
                //      thread 0's first pixel, so the prefix scan carries it along the whole row.
                if (t == 0) v[0] = min(v[0], edge_l1 + LG_A5);
#pragma unroll
                for (int k = 1; k < E; k++) v[k] = min(v[k], v[k - 1] + LG_A5);
                int mloc = (int)v[E - 1] - (int)((uint32_t)(c0 + E - 1) * LG_A5);
                int pin = lg_wave_prefix_min(mloc);
                int excl = lg_wave_shr1(INT_MAX, pin);   // wave-local exclusive prefix
                // One LDS exchange per row: everything a neighbouring wave needs to rebuild this wave's border
                // pixels is published BEFORE the barrier (pre-carry values + prefixes); see "rotate" below.
                if (lane == 0) { s_x[par][wave][1] = (int)v[0]; s_x[par][wave][2] = (int)v[1]; }
                if (lane == 63) {
                    s_x[par][wave][0] = pin;
                    s_x[par][wave][3] = (int)v[E - 2]; s_x[par][wave][4] = (int)v[E - 1];
                    s_x[par][wave][5] = excl;
                }
                lg_lds_barrier();
                int wpre = INT_MAX, wpre_prev = INT_MAX;  // min of the totals of waves < wave, and < wave-1
#pragma unroll
                for (int w = 0; w < NW - 1; w++) {
                    const int tw = s_x[par][w][0];
                    if (w < wave) wpre = min(wpre, tw);
                    if (w < wave - 1) wpre_prev = min(wpre_prev, tw);
                }
                excl = min(excl, wpre);
                uint32_t cin = (t == 0) ? LG_INF : (uint32_t)(excl + (int)((uint32_t)(c0 - 1) * LG_A5));
#pragma unroll
                for (int k = 0; k < E; k++) v[k] = min(v[k], cin + (uint32_t)(k + 1) * LG_A5);
                // ---- write back
                const int prow = phys_row(r);
                if (!BWD) {
                    uint32_t* dst = tp + (size_t)prow * W + pc0;
                    if (full) {
#pragma unroll
                        for (int q = 0; q < E / 4; q++)
                            *reinterpret_cast<uint4*>(dst + 4 * q) =
                                make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < E; k++)
                            if (pc0 + k < W) dst[k] = v[k];
                    }
                } else {
                    float o[E];
#pragma unroll
                    for (int k = 0; k < E; k++) {
                        const int pc = pc0 + (E - 1 - k);
                        uint32_t val = v[k];
                        // OpenCV's border cells (lg_dt_far): all there is in an image without any source pixel (no path: >= LG_INF)
                        if (far || val >= LG_INF) {
                            int dd = min(min(pc + 1, W - pc), min(prow + 1, H - prow));
                            const uint32_t cap = init0 + (uint32_t)dd * LG_A5;
                            val = val >= LG_INF ? cap : min(val, cap);
                        }
                        if (pc < W) mx = max(mx, val);
                        o[E - 1 - k] = (float)val * (1.0f / 65536.0f);
                    }
                    if (dout) {
                        float* dst = dout + (size_t)prow * W + pc0;
                        if (full) {
#pragma unroll
                            for (int q = 0; q < E / 4; q++)
                                *reinterpret_cast<float4*>(dst + 4 * q) =
                                    make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
                        } else {
#pragma unroll
                            for (int k = 0; k < E; k++)
                                if (pc0 + k < W) dst[k] = o[k];
                        }
                    }
                }
                // ---- rotate row registers, exchange 2-column halos with the neighbouring threads
#pragma unroll
                for (int j = 0; j < E + 2; j++) p2[j] = p1[j + 1];
                uint32_t l0 = (uint32_t)lg_wave_shr1((int)LG_INF, (int)v[E - 2]);
                uint32_t l1 = (uint32_t)lg_wave_shr1((int)LG_INF, (int)v[E - 1]);
                uint32_t r0 = (uint32_t)lg_wave_shl1((int)LG_INF, (int)v[0]);
                uint32_t r1 = (uint32_t)lg_wave_shl1((int)LG_INF, (int)v[1]);
                if (lane == 0 && wave > 0) {
                    // final values of thread t-1 (lane 63 of the previous wave), rebuilt from what it published
                    const int exl = min(s_x[par][wave - 1][5], wpre_prev);
                    const uint32_t cprev = (uint32_t)(exl + (int)((uint32_t)(c0 - E - 1) * LG_A5));
                    l0 = min((uint32_t)s_x[par][wave - 1][3], cprev + (uint32_t)(E - 1) * LG_A5);
                    l1 = min((uint32_t)s_x[par][wave - 1][4], cprev + (uint32_t)E * LG_A5);
                }
                if (t == 0) { l0 = edge_l2; l1 = edge_l1; }
                if (lane == 63 && wave == nwa - 1) { r0 = edge_r0; r1 = edge_r1; }
                if (lane == 63 && wave < nwa - 1) {
                    // final values of thread t+1 (lane 0 of the next wave): its carry is the prefix over all threads <= t
                    const int inc = min(s_x[par][wave][0], wpre);
                    const uint32_t cnext = (uint32_t)(inc + (int)((uint32_t)(c0 + E - 1) * LG_A5));
                    r0 = min((uint32_t)s_x[par][wave + 1][1], cnext + LG_A5);
                    r1 = min((uint32_t)s_x[par][wave + 1][2], cnext + 2u * LG_A5);
                }
                p1[0] = l0; p1[1] = l1;
#pragma unroll
                for (int k = 0; k < E; k++) p1[2 + k] = v[k];
                p1[E + 2] = r0; p1[E + 3] = r1;
            }
        }
#pragma unroll
        for (int d = 0; d < D; d++)
#pragma unroll
            for (int q = 0; q < RAWN; q++) raw[d][q] = nxt[d][q];
    }
    if (BWD) {
        mx = lg_wave_max_u32(mx);
        if (lane == 0) atomicMax(&maxfix[frame * LG_MF + which], mx);
    }
}

template <int T, int E>
static void lg_dt_launch_t(bool bwd, const uint8_t* mask, uint32_t* tmp, float* dist_out, uint32_t* maxfix,
                           const LgWin* win, int B, int H, int W, uint32_t init0, hipStream_t s) {
    dim3 grid(2, B), block(T);
    const bool vec = (W % E) == 0 && W >= E;
    if (bwd) {
        if (vec) hipLaunchKernelGGL((lg_dt5_kernel<T, E, true, true>), grid, block, 0, s, mask, tmp, dist_out, maxfix, win, H, W, init0);
        else hipLaunchKernelGGL((lg_dt5_kernel<T, E, true, false>), grid, block, 0, s, mask, tmp, dist_out, maxfix, win, H, W, init0);
    } else {
        if (vec) hipLaunchKernelGGL((lg_dt5_kernel<T, E, false, true>), grid, block, 0, s, mask, tmp, dist_out, maxfix, win, H, W, init0);
        else hipLaunchKernelGGL((lg_dt5_kernel<T, E, false, false>), grid, block, 0, s, mask, tmp, dist_out, maxfix, win, H, W, init0);
    }
}

// threads x columns-per-thread of the sweep workgroup for width W: returns 64 * E, *waves = T / 64 (0: unsupported)
int lg_dt_geometry(int W, int* waves) {
    int T, E;
    if (W <= 2048) {
        E = 4;
        T = W <= 256 ? 64 : W <= 512 ? 128 : W <= 1024 ? 256 : 512;
    } else {
        E = 8;
        T = W <= 4096 ? 512 : W <= 8192 ? 1024 : 0;
    }
    if (waves) *waves = T / 64;
    return T ? 64 * E : 0;
}

int lg_launch_dt(bool bwd, const uint8_t* mask, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                 int H, int W, uint32_t init0, hipStream_t s) {
    // threads * E columns must cover the row.  E = 4 keeps the per-row dependency chain short (best up to
    // 2048 columns: 0.70/0.82 ms vs 0.82/0.91 ms at 1080p); at 4K 512x8 beats 1024x4 (2.04/2.54 vs 2.65/3.12 ms).
    if (W <= 256) lg_dt_launch_t<64, 4>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);
    else if (W <= 512) lg_dt_launch_t<128, 4>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);
    else if (W <= 1024) lg_dt_launch_t<256, 4>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);
    else if (W <= 2048) lg_dt_launch_t<512, 4>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);
    else if (W <= 4096) lg_dt_launch_t<512, 8>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);   // 4K: 8 waves beat 16 (measured)
    else if (W <= 8192) lg_dt_launch_t<1024, 8>(bwd, mask, tmp, dist_out, maxfix, win, B, H, W, init0, s);
    else return -1;
    return 0;
}

// ============================================================================ d_in without the sweeps: run distances + row search
// The two raster passes of the 5x5 chamfer transform give  d(p) = min over zero pixels q of N(p - q)  with the closed-form
// chamfer norm N (LgWin; pinned in tests/test_oracle_c.py), and N is monotone in |dx| and in |dy|.  For a fixed row y' only the
// zero pixel of that row nearest to column x can matter:
//     d(x, y) = min over rows y' of N(h[y'][x], |y - y'|),   h[y'][x] = distance from x to the nearest zero pixel of row y'
// h comes straight from the bit rows (count-leading/trailing-zeros, no sequential dependence: lg_hrun_kernel); the search over
// rows is bounded by N(., dy) >= a * dy: rows further away than the best value found so far cannot improve it
// (lg_dtsearch_kernel).  Every leaf pixel is independent -- the work spreads over all CUs instead of one workgroup per frame
// walking the window's rows one after the other (~1 us per row).  Rows outside [by0 - 1, by1 + 1] never matter: the rows next
// to the bounding box are all zero (h = 0) and nearer than any row beyond them.  Out-of-image pixels are not sources.
// Both kernels: workgroup ids are dealt round-robin to the 8 XCDs, and a frame's workgroups all carry the same id % 8, so a
// frame's run distances are written and read through ONE XCD's L2.  grid = 8 * G * ceil(B / 8).
__device__ __forceinline__ bool lg_frame_of_block(int G, int B, int* frame, int* j) {
    const int id = (int)blockIdx.x, q = id >> 3;
    const int fq = q / G;
    *frame = (id & 7) + 8 * fq;
    *j = q - fq * G;
    return *frame < B;
}

__device__ __forceinline__ unsigned long long lg_readlane_u64(unsigned long long v, int l) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
// One wave per row of [by0 - 1, by1 + 1]: lane k loads word k of the bounding box (one coalesced load, nothing else is read:
// in-image words outside the bounding box are all zero pixels), the nearest word with a zero pixel on either side of a word
// comes from a ballot, and the row's words are then written one after the other, lane = pixel.  Rows wider than 64 words
// (W > 4096 and a leaf spanning them) are processed in 64-word pieces whose neighbours are looked up in memory.
__global__ __launch_bounds__(256) void lg_hrun_kernel(const unsigned long long* __restrict__ bits, const LgWin* __restrict__ wins,
                                                      uint32_t* __restrict__ tmp, int H, int W, int WW, int G, int B) {
    int frame, j;
    if (!lg_frame_of_block(G, B, &frame, &j)) return;
    const LgWin w = wins[frame];
    if (!w.search_in) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = max(w.by0 - 1, 0), r1 = min(w.by1 + 1, H - 1);
    const int w0 = w.bx0 >> 6, w1 = w.bx1 >> 6;
    const unsigned long long* fb = bits + (size_t)frame * H * WW;
    uint16_t* hd = reinterpret_cast<uint16_t*>(tmp + (size_t)frame * 2 * H * W);
    const int tail = W & 63;   // the last word's bits beyond the image are neither leaf nor source
    for (int y = r0 + j * 4 + wave; y <= r1; y += 4 * G) {
        const unsigned long long* row = fb + (size_t)y * WW;
        auto zeros = [&](int k) -> unsigned long long {   // zero pixels of word k (k in [0, WW))
            unsigned long long z = ~row[k];
            if (k == WW - 1 && tail) z &= (1ull << tail) - 1ull;
            return z;
        };
        for (int c0 = w0; c0 <= w1; c0 += 64) {
            const int nc = min(64, w1 - c0 + 1);
            const unsigned long long z = lane < nc ? zeros(c0 + lane) : 0ull;
            const unsigned long long nz = __ballot(z != 0ull);
            // nearest zero pixel left of the piece's first pixel / right of its last one, as distances from those pixels
            unsigned edge_l = LG_HCAP, edge_r = LG_HCAP;
            for (int k = c0 - 1; k >= 0; k--) {
                const unsigned long long zk = zeros(k);
                if (zk) { edge_l = 64u * (unsigned)(c0 - 1 - k) + (unsigned)__builtin_clzll(zk) + 1u; break; }
            }
            for (int k = c0 + nc; k < WW; k++) {
                const unsigned long long zk = zeros(k);
                if (zk) { edge_r = 64u * (unsigned)(k - c0 - nc) + (unsigned)__builtin_ctzll(zk) + 1u; break; }
            }
            for (int i = 0; i < nc; i++) {
                const unsigned long long zi = lg_readlane_u64(z, i);
                const unsigned long long ml = i ? nz & ((1ull << i) - 1ull) : 0ull, mr = i < 63 ? nz >> (i + 1) : 0ull;
                unsigned lc, rc;
                if (ml) {
                    const int k = 63 - __builtin_clzll(ml);
                    lc = 64u * (unsigned)(i - 1 - k) + (unsigned)__builtin_clzll(lg_readlane_u64(z, k)) + 1u;
                } else {
                    lc = min(LG_HCAP, 64u * (unsigned)i + edge_l);
                }
                if (mr) {
                    const int k = i + 1 + __builtin_ctzll(mr);
                    rc = 64u * (unsigned)(k - i - 1) + (unsigned)__builtin_ctzll(lg_readlane_u64(z, k)) + 1u;
                } else {
                    rc = min(LG_HCAP, 64u * (unsigned)(nc - 1 - i) + edge_r);
                }
                const unsigned long long zl = zi << (63 - lane);   // pixels <= lane, the pixel itself in bit 63
                const unsigned long long zr = zi >> lane;          // pixels >= lane, the pixel itself in bit 0
                const unsigned dl = zl ? (unsigned)__builtin_clzll(zl) : (unsigned)lane + lc;
                const unsigned dr = zr ? (unsigned)__builtin_ctzll(zr) : (unsigned)(63 - lane) + rc;
                const int x = 64 * (c0 + i) + lane;
                if (x < W) hd[(unsigned)(y * W) + (unsigned)x] = (uint16_t)min(min(dl, dr), LG_HCAP);
            }
        }
    }
}

// N(h, dy) as the maximum of its four linear pieces (a norm is the maximum of its supporting functionals; for this mask
// 2a <= c <= a + b makes them a*M + (c-2a)*m and (c-b)*M + (2b-c)*m with M, m the larger / smaller of the two arguments):
// dy is wave-uniform, so its four products live in scalar registers and a candidate costs four 24-bit multiply-adds.
#define LG_N5_AL (LG_C5 - 2u * LG_A5)   // 12904
#define LG_N5_BE (LG_C5 - LG_B5)        // 52226
#define LG_N5_GA (2u * LG_B5 - LG_C5)   // 39524
struct LgH4 { uint32_t a, al, be, ga; };   // h times the four coefficients: shared by the lane's four pixels
__device__ __forceinline__ LgH4 lg_h4(uint32_t h) {   // h <= LG_HCAP
    LgH4 r = {h << 16, (uint32_t)__umul24(h, LG_N5_AL), (uint32_t)__umul24(h, LG_N5_BE), (uint32_t)__umul24(h, LG_N5_GA)};
    // (keeps the three products: hipcc otherwise re-fuses them into one multiply-add per pixel whose scalar addend costs a move)
    asm volatile("" : "+v"(r.al), "+v"(r.be), "+v"(r.ga));
    return r;
}
__device__ __forceinline__ uint32_t lg_norm5_h(const LgH4& h, uint32_t dy) {   // dy <= 16384 (wave-uniform): below 2^32
    const uint32_t t0 = h.a + __umul24(dy, LG_N5_AL);
    const uint32_t t1 = h.al + (dy << 16);
    const uint32_t t2 = h.be + __umul24(dy, LG_N5_GA);
    const uint32_t t3 = h.ga + __umul24(dy, LG_N5_BE);
    return max(max(t0, t1), max(t2, t3));
}

// Workgroup = one 64 x 16 tile of the window at a time (the score-plane kernel's tiles), wave = 4 rows, lane = column: a
// candidate row's h is loaded once (128 contiguous bytes per wave) and serves the lane's four pixels.
__global__ __launch_bounds__(256) void lg_dtsearch_kernel(const unsigned long long* __restrict__ bits,
                                                          const LgWin* __restrict__ wins, const uint32_t* __restrict__ tmp,
                                                          float* __restrict__ dist_out, uint32_t* __restrict__ maxfix, int H,
                                                          int W, int WW, int wc, int G, int B) {
    int frame, j;
    if (!lg_frame_of_block(G, B, &frame, &j)) return;
    const LgWin w = wins[frame];
    if (!w.search_in) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wxe = min(W, w.wx0 + w.nw * wc);
    const int ntx = (wxe - w.wx0 + 63) >> 6, nty = (w.wy1 - w.wy0 + LG_TH - 1) / LG_TH;
    const int lo = max(w.by0 - 1, 0), hi = min(w.by1 + 1, H - 1);   // candidate rows
    const unsigned long long* fb = bits + (size_t)frame * H * WW;
    const uint16_t* hd = reinterpret_cast<const uint16_t*>(tmp + (size_t)frame * 2 * H * W);
    float* dout = dist_out + (size_t)frame * H * W;
    uint32_t mx = 0;
    static_assert(LG_TH == 16, "four waves x four rows");
    const int ntile = __builtin_amdgcn_readfirstlane(ntx * nty);
    for (int tile = j; tile < ntile; tile += G) {
        const int tyi = __builtin_amdgcn_readfirstlane(tile / ntx), txi = tile - tyi * ntx;
        const int wi = (w.wx0 >> 6) + txi;
        const int x = 64 * wi + lane, yb = w.wy0 + LG_TH * tyi + 4 * wave;
        const bool xin = x < W;
        const unsigned xc = (unsigned)min(x, W - 1);
        unsigned long long rb[4];   // the tile is word aligned: one word per row, the same for every lane
#pragma unroll
        for (int i = 0; i < 4; i++) rb[i] = fb[(unsigned)(min(yb + i, H - 1) * WW + wi)];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            rb[i] = yb + i < H ? rb[i] : 0ull;
            rb[i] = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rb[i] >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)rb[i]);
        }
        if (!(rb[0] | rb[1] | rb[2] | rb[3])) {   // no leaf pixel in these four rows: d_in = 0
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (xin && yb + i < H) dout[(unsigned)((yb + i) * W) + xc] = 0.0f;
            continue;
        }
        uint32_t best[4];
#pragma unroll
        for (int i = 0; i < 4; i++) best[i] = (xin && ((rb[i] >> lane) & 1ull)) ? 0xFFFFFFFFu : 0u;
        // the four rows themselves (a leaf pixel's own row always lies in [lo, hi]; rows beyond have no leaf pixel and, as
        // candidates, lose to the all-zero rows lo / hi)
        {
            uint32_t h4[4];
#pragma unroll
            for (int i2 = 0; i2 < 4; i2++) h4[i2] = hd[(unsigned)(max(lo, min(yb + i2, hi)) * W) + xc];
#pragma unroll
            for (int i2 = 0; i2 < 4; i2++) {
                if (yb + i2 >= lo && yb + i2 <= hi) {
                    const LgH4 hh = lg_h4(h4[i2]);
#pragma unroll
                    for (int i = 0; i < 4; i++) best[i] = min(best[i], lg_norm5_h(hh, (uint32_t)(i > i2 ? i - i2 : i2 - i)));
                }
            }
        }
        // rows above (yb - k) and below (yb + 3 + k), four steps per round so that eight loads are in flight
        for (int k0 = 1;; k0 += 4) {
            const int yu0 = yb - k0, yd0 = yb + 3 + k0;
            if (yu0 < lo && yd0 > hi) break;
            const uint32_t bm = max(max(best[0], best[1]), max(best[2], best[3]));
            if (!__any((uint32_t)k0 * LG_A5 < bm)) break;   // N(., dy) >= a * dy >= a * k0 from here on
            uint32_t hu[4], hv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                hu[q] = hd[(unsigned)(max(yu0 - q, lo) * W) + xc];
                hv[q] = hd[(unsigned)(min(yd0 + q, hi) * W) + xc];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t k = (uint32_t)(k0 + q);
                const uint32_t bq = max(max(best[0], best[1]), max(best[2], best[3]));
                // a row whose h is at least the best value everywhere in the wave cannot improve anything: N(h, .) >= a * h
                if (yu0 - q >= lo && __any((hu[q] << 16) < bq)) {
                    const LgH4 hh = lg_h4(hu[q]);
#pragma unroll
                    for (int i = 0; i < 4; i++) best[i] = min(best[i], lg_norm5_h(hh, k + (uint32_t)i));
                }
                if (yd0 + q <= hi && __any((hv[q] << 16) < bq)) {
                    const LgH4 hh = lg_h4(hv[q]);
#pragma unroll
                    for (int i = 0; i < 4; i++) best[i] = min(best[i], lg_norm5_h(hh, k + (uint32_t)(3 - i)));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            mx = max(mx, best[i]);
            if (xin && yb + i < H) dout[(unsigned)((yb + i) * W) + xc] = (float)best[i] * (1.0f / 65536.0f);
        }
    }
    mx = lg_wave_max_u32(mx);
    if (lane == 0 && mx) atomicMax(&maxfix[frame * LG_MF + 0], mx);
}

// ---- the seed rows of form 5 (lg_dtband_kernel).  The same bounded search as lg_dtsearch_kernel, on pairs of adjacent rows P
// apart only: a lane's NP = 4 rows are two pairs, ya0 + P i and ya0 + P i + 1, so a candidate row's load serves four pixels.
// The scan goes outwards from the middle of the lane's rows, c - k and c + 1 + k: every row of the lane lies within SPAN rows of
// c, N(., dy) >= a * dy, so once a * (k - SPAN) reaches the largest value any lane still holds no further row can improve one
// and the scan stops.  The results go to distance_map and, as 16.16 integers, to the seed rows (lg_dt_seed_rows), pair i of the
// window in rows 2 i and 2 i + 1 -- the integers seed the bands, not distance_map's floats, which are not exact above 2^24.
__device__ __forceinline__ uint32_t* lg_dt_seed_rows(uint32_t* tmp, int frame, int H, int W) {
    // the half of the frame's d_in workspace behind the run distances ([H][W] uint16), 16-byte aligned
    return tmp + (size_t)frame * 2 * H * W + ((((size_t)H * W + 1) / 2 + 3) & ~(size_t)3);
}
template <int P>
__global__ __launch_bounds__(256) void lg_dtseed_kernel(const unsigned long long* __restrict__ bits,
                                                        const LgWin* __restrict__ wins, uint32_t* __restrict__ tmp,
                                                        float* __restrict__ dist_out, uint32_t* __restrict__ maxfix, int H,
                                                        int W, int WW, int wc, int G, int B) {
    int frame, j;
    if (!lg_frame_of_block(G, B, &frame, &j)) return;
    const LgWin w = wins[frame];
    if (!w.search_in) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wxe = min(W, w.wx0 + w.nw * wc);
    static_assert(P >= 4, "pairs of adjacent rows, P apart");
    constexpr int NP = 4, NG = NP / 2;   // rows, pairs per lane
    constexpr int ROWS = 4 * NG * P;     // rows per workgroup tile: four waves x NG pairs x P
    auto roff = [](int i) { return P * (i >> 1) + (i & 1); };   // the lane's i-th row, from ya0
    const int ntx = (wxe - w.wx0 + 63) >> 6, nty = (w.wy1 - w.wy0 + ROWS - 1) / ROWS;
    const int lo = max(w.by0 - 1, 0), hi = min(w.by1 + 1, H - 1);   // candidate rows
    const unsigned long long* fb = bits + (size_t)frame * H * WW;
    const uint16_t* hd = reinterpret_cast<const uint16_t*>(tmp + (size_t)frame * 2 * H * W);
    uint32_t* seed = lg_dt_seed_rows(tmp, frame, H, W);   // [seed row][W]
    float* dout = dist_out + (size_t)frame * H * W;
    uint32_t mx = 0;
    constexpr int SPAN = (P * (NG - 1) + 1) / 2;   // the lane's rows lie within SPAN rows of the scan's centre
    const int ntile = __builtin_amdgcn_readfirstlane(ntx * nty);
    for (int tile = j; tile < ntile; tile += G) {
        const int tyi = __builtin_amdgcn_readfirstlane(tile / ntx), txi = tile - tyi * ntx;
        const int wi = (w.wx0 >> 6) + txi;
        const int x = 64 * wi + lane, ya0 = w.wy0 + ROWS * tyi + P * NG * wave;
        if (ya0 >= w.wy1) continue;   // (wave-uniform)
        const bool xin = x < W;
        const unsigned xc = (unsigned)min(x, W - 1);
        unsigned long long rb[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int y = ya0 + roff(i);
            rb[i] = fb[(unsigned)(min(y, H - 1) * WW + wi)];
            rb[i] = y < w.wy1 ? lg_readlane_u64(rb[i], 0) : 0ull;
        }
        unsigned long long anyb = 0;
#pragma unroll
        for (int i = 0; i < NP; i++) anyb |= rb[i];
        uint32_t best[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) best[i] = (xin && ((rb[i] >> lane) & 1ull)) ? 0xFFFFFFFFu : 0u;
        if (anyb) {
            const int c = ya0 + SPAN;   // scan outwards from here: rows c - k and c + 1 + k
            for (int k0 = 0;; k0 += 4) {
                const int yu0 = c - k0, yd0 = c + 1 + k0;
                if (yu0 < lo && yd0 > hi) break;
                uint32_t bm = best[0];
#pragma unroll
                for (int i = 1; i < NP; i++) bm = max(bm, best[i]);
                if (!__any((uint32_t)max(k0 - SPAN, 0) * LG_A5 < bm)) break;   // every row of the lane is at least k0 - SPAN rows away from here on
                uint32_t hu[4], hv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    hu[q] = hd[(unsigned)(min(max(yu0 - q, lo), hi) * W) + xc];
                    hv[q] = hd[(unsigned)(max(min(yd0 + q, hi), lo) * W) + xc];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    uint32_t bq = best[0];
#pragma unroll
                    for (int i = 1; i < NP; i++) bq = max(bq, best[i]);
                    const int yu = yu0 - q, yd = yd0 + q;
                    if (yu >= lo && yu <= hi && __any((hu[q] << 16) < bq)) {
                        const LgH4 hh = lg_h4(hu[q]);
#pragma unroll
                        for (int i = 0; i < NP; i++) {
                            const int dy = ya0 + roff(i) - yu;
                            best[i] = min(best[i], lg_norm5_h(hh, (uint32_t)(dy < 0 ? -dy : dy)));
                        }
                    }
                    if (yd >= lo && yd <= hi && __any((hv[q] << 16) < bq)) {
                        const LgH4 hh = lg_h4(hv[q]);
#pragma unroll
                        for (int i = 0; i < NP; i++) {
                            const int dy = ya0 + roff(i) - yd;
                            best[i] = min(best[i], lg_norm5_h(hh, (uint32_t)(dy < 0 ? -dy : dy)));
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int y = ya0 + roff(i);
            mx = max(mx, best[i]);
            if (xin && y < w.wy1) {
                dout[(unsigned)(y * W) + xc] = (float)best[i] * (1.0f / 65536.0f);
                seed[(size_t)(2 * ((ya0 - w.wy0) / P + (i >> 1)) + (i & 1)) * W + xc] = best[i];
            }
        }
    }
    mx = lg_wave_max_u32(mx);
    if (lane == 0 && mx) atomicMax(&maxfix[frame * LG_MF + 0], mx);
}

// ---- the rows between two seed pairs by the 5 x 5 stencil itself (tests/test_dt_band_math.py).  With h the run distance of a
// pixel's own row,  U(y, x) = min(A h[y][x], U(y-1, x) + A, min U(y-1, x+-1) + B, min(U(y-1, x+-2), U(y-2, x+-1)) + C)  is the
// distance to the nearest zero pixel at or above row y: an optimal chamfer path uses at most two adjacent generators in any
// order, so its horizontal steps can all be taken along the source's own row (A h) and nothing is left to scan within the row.
// Started from the TRUE d on the pair above a band and run downwards, and mirrored from the pair below and run upwards, the
// minimum of the two is the true d on every row between: a seed is an upper bound the triangle inequality keeps valid, every
// path from outside the band crosses a pair (a knight's move skips at most one row), sources inside enter through A h.
// Wave = the P - 2 rows between the pairs at window rows P k and P (k + 1), times 64 E columns, lane = E columns, everything in
// registers: no LDS, no barrier, nothing waits for another wave.  A stencil step reaches two columns sideways, so what a wave
// computes is exact 2 (P - 2) columns inside its ends: neighbouring waves overlap by that much on either side and store only
// their centre.  Rows and columns outside the window are off the leaf (d = h = 0) inside the image and "no path" outside it.
// The row step itself, lane = E consecutive columns (lg_dtband_kernel, lg_dtsweep_kernel): p1 = the row one step back (columns
// -2 .. E + 1 of the lane), p2 = the one before (-1 .. E); the halo comes from the neighbouring lanes by wave shifts.  fl: what
// lane 0 sees in the columns left of its own, fr0 / fr1: what lane 63 sees in the two columns right of its own.
template <int E>
struct LgRowStep {
    uint32_t p1[E + 4], p2[E + 2];
    __device__ __forceinline__ void set_p1(const uint32_t* v, uint32_t fl, uint32_t fr0, uint32_t fr1) {
        p1[0] = (uint32_t)lg_wave_shr1((int)fl, (int)v[E - 2]);
        p1[1] = (uint32_t)lg_wave_shr1((int)fl, (int)v[E - 1]);
#pragma unroll
        for (int k = 0; k < E; k++) p1[2 + k] = v[k];
        p1[E + 2] = (uint32_t)lg_wave_shl1((int)fr0, (int)v[0]);
        p1[E + 3] = (uint32_t)lg_wave_shl1((int)fr1, (int)v[1]);
    }
    __device__ __forceinline__ void set_p2(const uint32_t* v, uint32_t fl, uint32_t fr0) {
        p2[0] = (uint32_t)lg_wave_shr1((int)fl, (int)v[E - 1]);
#pragma unroll
        for (int k = 0; k < E; k++) p2[1 + k] = v[k];
        p2[E + 1] = (uint32_t)lg_wave_shl1((int)fr0, (int)v[0]);
    }
    // one row of the recurrence from A h of the row (two columns per register, uint16), then the row registers move on
    __device__ __forceinline__ void step(const uint32_t* hpi, uint32_t* v, uint32_t fl, uint32_t fr0, uint32_t fr1) {
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint32_t ah = (k & 1) ? (hpi[k >> 1] & 0xFFFF0000u) : (hpi[k >> 1] << 16);
            // equal weights are grouped before they are added: min(x + w, y + w) == min(x, y) + w (values < 2^31)
            const uint32_t mc = min(min(p2[k], p2[k + 2]), min(p1[k], p1[k + 4])) + LG_C5;
            const uint32_t mb = min(p1[k + 1], p1[k + 3]) + LG_B5;
            const uint32_t ma = p1[k + 2] + LG_A5;
            v[k] = min(min(mc, mb), min(ma, ah));
        }
#pragma unroll
        for (int q = 0; q < E + 2; q++) p2[q] = p1[q + 1];
        set_p1(v, fl, fr0, fr1);
    }
};

template <int P, int E, bool VEC>   // VEC: W % E == 0, a lane's E columns are one aligned load / store
__global__ __launch_bounds__(256) void lg_dtband_kernel(const unsigned long long* __restrict__ bits,
                                                        const LgWin* __restrict__ wins, uint32_t* __restrict__ tmp,
                                                        float* __restrict__ dist_out, uint32_t* __restrict__ maxfix, int H, int W,
                                                        int WW, int wc, int G, int B) {
    constexpr int N = P - 2, HALO = 2 * N, WCOL = 64 * E, S = WCOL - 2 * HALO, EH = E / 2;
    static_assert((E == 2 || E == 4) && S > 0 && HALO % E == 0, "whole lanes of halo on either side of a centre");
    constexpr uint32_t HOUT = LG_HCAP;   // h outside the image: like a row without a zero pixel, an upper bound that beats nothing
    int frame, j;
    if (!lg_frame_of_block(G, B, &frame, &j)) return;
    const LgWin w = wins[frame];
    if (!w.search_in) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wxe = min(W, w.wx0 + w.nw * wc);
    const int ntx = (wxe - w.wx0 + S - 1) / S, nby = (w.wy1 - w.wy0 - 2 + P - 1) / P;   // band k: rows wy0 + P k + 2 ... < wy1
    const int r0 = max(w.by0 - 1, 0), r1 = min(w.by1 + 1, H - 1);                  // rows and
    const int hx0 = (w.bx0 >> 6) << 6, hx1 = min(W, ((w.bx1 >> 6) + 1) << 6);     // columns lg_hrun_kernel wrote
    const uint16_t* hd = reinterpret_cast<const uint16_t*>(tmp + (size_t)frame * 2 * H * W);
    const uint32_t* seed = lg_dt_seed_rows(tmp, frame, H, W);
    float* dout = dist_out + (size_t)frame * H * W;
    const bool centre = lane * E >= HALO && lane * E < WCOL - HALO;
    uint32_t mx = 0;
    const int nunit = __builtin_amdgcn_readfirstlane(ntx * nby);
    for (int u = 4 * j + wave; u < nunit; u += 4 * G) {
        const int byi = __builtin_amdgcn_readfirstlane(u / ntx), txi = u - byi * ntx;
        const int s = w.wy0 + P * byi + 2;               // first row of the band
        const int xl = w.wx0 + S * txi - HALO + E * lane;   // the lane's first column
        const bool lane_in = xl >= 0 && xl + E <= W;     // (VEC: a lane lies in the image or outside it)
        auto col_in = [&](int k) { return VEC ? lane_in : (xl + k >= 0 && xl + k < W); };
        auto store_row = [&](int y, const uint32_t* v) {   // the centre's columns inside the window; y < wy1
            float* dst = dout + (size_t)y * W + xl;
            if (VEC) {
                if (centre && xl + E <= wxe) {
                    if (E == 4) *reinterpret_cast<float4*>(dst) = make_float4((float)v[0] * (1.0f / 65536.0f), (float)v[1] * (1.0f / 65536.0f),
                                                                               (float)v[2] * (1.0f / 65536.0f), (float)v[E - 1] * (1.0f / 65536.0f));
                    else *reinterpret_cast<float2*>(dst) = make_float2((float)v[0] * (1.0f / 65536.0f), (float)v[1] * (1.0f / 65536.0f));
#pragma unroll
                    for (int k = 0; k < E; k++) mx = max(mx, v[k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < E; k++)
                    if (centre && xl + k < wxe) {
                        dst[k] = (float)v[k] * (1.0f / 65536.0f);
                        mx = max(mx, v[k]);
                    }
            }
        };
        const uint32_t zero[E] = {};
        // a band or a centre beside the bounding box holds no leaf pixel
        const int xc0 = w.wx0 + S * txi;
        bool leaf = s <= w.by1 && s + N > w.by0 && xc0 <= w.bx1 && xc0 + S > w.bx0;
        // ---- A h of the band's rows, two columns per register (uint16 as lg_hrun_kernel wrote them)
        uint32_t hp[N][EH];
        if (leaf) {
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < N; i++) {
                const int y = s + i;
                const bool yin = y < H, hrow = y >= r0 && y <= r1;   // (y >= wy0 + 2)
                const uint16_t* row = hd + (size_t)(hrow ? y : r0) * W;
                if (VEC) {
                    const bool ld = hrow && lane_in && xl >= hx0 && xl < hx1;
                    const uint16_t* src = row + (ld ? xl : 0);
                    uint32_t raw[EH];
                    if (E == 4) { const uint2 v = *reinterpret_cast<const uint2*>(src); raw[0] = v.x; raw[EH - 1] = v.y; }
                    else raw[0] = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
                    for (int q = 0; q < EH; q++) hp[i][q] = ld ? raw[q] : ((yin && lane_in) ? 0u : (HOUT | (HOUT << 16)));
                } else {
                    uint32_t hv[E];
#pragma unroll
                    for (int k = 0; k < E; k++) {
                        const int c = xl + k;
                        const bool ld = hrow && c >= hx0 && c < hx1;   // (inside the image)
                        const uint32_t v = row[ld ? c : 0];
                        hv[k] = ld ? v : ((yin && col_in(k)) ? 0u : HOUT);
                    }
#pragma unroll
                    for (int q = 0; q < EH; q++) hp[i][q] = hv[2 * q] | (hv[2 * q + 1] << 16);
                }
                if (y < w.wy1) {
#pragma unroll
                    for (int q = 0; q < EH; q++) any |= hp[i][q];
                }
            }
            // h > 0 is a leaf pixel (the centre's columns of rows < wy1 lie in the image unless they are past the window's end)
            leaf = __any(centre && xl < wxe && any != 0u);
        }
        if (!leaf) {
#pragma unroll
            for (int i = 0; i < N; i++)
                if (s + i < w.wy1) store_row(s + i, zero);
            continue;
        }
        // ---- a seed row (any row index: true d where it was searched, else off the leaf / outside the image)
        auto load_seed = [&](int y, uint32_t* dst) {
            const bool yin = y >= 0 && y < H;
            if (y < w.wy0 || y >= w.wy1) {   // (wave-uniform)
#pragma unroll
                for (int k = 0; k < E; k++) dst[k] = (yin && col_in(k)) ? 0u : LG_INF;
                return;
            }
            const int rel = y - w.wy0;
            const uint32_t* row = seed + (size_t)(2 * (rel / P) + rel % P) * W;
            if (VEC) {
                const bool ld = lane_in && xl >= w.wx0 && xl < wxe;
                const uint32_t* src = row + (ld ? xl : 0);
                uint32_t raw[E];
                if (E == 4) { const uint4 v = *reinterpret_cast<const uint4*>(src); raw[0] = v.x; raw[1] = v.y; raw[E - 2] = v.z; raw[E - 1] = v.w; }
                else { const uint2 v = *reinterpret_cast<const uint2*>(src); raw[0] = v.x; raw[1] = v.y; }
#pragma unroll
                for (int k = 0; k < E; k++) dst[k] = ld ? raw[k] : (lane_in ? 0u : LG_INF);
            } else {
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const int c = xl + k;
                    const bool ld = c >= w.wx0 && c < wxe;
                    const uint32_t v = row[ld ? c : 0];
                    dst[k] = ld ? v : (col_in(k) ? 0u : LG_INF);
                }
            }
        };
        LgRowStep<E> rs;   // (beyond the wave's ends: "no path" -- the halo absorbs it)
        auto start = [&](int y2, int y1) {   // p2 / p1 from the seed rows two steps / one step back
            uint32_t v[E];
            load_seed(y2, v);
            rs.set_p2(v, LG_INF, LG_INF);
            load_seed(y1, v);
            rs.set_p1(v, LG_INF, LG_INF, LG_INF);
        };
        auto step = [&](const uint32_t* hpi, uint32_t* v) { rs.step(hpi, v, LG_INF, LG_INF, LG_INF); };
        uint32_t res[N][E];
        start(s - 2, s - 1);
#pragma unroll
        for (int i = 0; i < N; i++) step(hp[i], res[i]);
        start(s + N + 1, s + N);
#pragma unroll
        for (int i = N - 1; i >= 0; i--) {
            uint32_t v[E];
            step(hp[i], v);
#pragma unroll
            for (int k = 0; k < E; k++) v[k] = min(v[k], res[i][k]);
            if (s + i < w.wy1) store_row(s + i, v);
        }
    }
    mx = lg_wave_max_u32(mx);
    if (lane == 0 && mx) atomicMax(&maxfix[frame * LG_MF + 0], mx);
}

// ---- form 6: the same row step over the whole bounding box, one workgroup per frame and no seed rows at all.  Wave 0 runs U
// downwards from the box's first row, wave 1 runs D upwards from its last row, both over the span of 64 E columns that holds the
// box (E = 4, 8, 16 or 32: W <= 2048), lane = E columns in registers.  Rows above / below the box and columns beside the span
// are off the leaf: 0 inside the image, "no path" outside it.  The waves meet at mid-height: up to there each stores its own
// exact 16.16 row, one workgroup barrier follows, and past it each takes the minimum with the row the other stored and writes
// the float.  The rows are parked in distance_map itself, in the very words the final floats replace (every word is read and
// then rewritten by the same lane): the seed-row area of `tmp` holds H / 2 rows and a box may be as high as the frame.  Waves
// 2 and 3 meanwhile write the 0 of the window's cells outside the box's rows and the span.  h rows do not depend on each other:
// PF rows of loads stay in flight (their out-of-range columns are replaced when a row is used, not when it is loaded).
template <int E, bool VEC>   // VEC: W % 4 == 0, four columns are one aligned load / store
__device__ __forceinline__ void lg_dtsweep_body(const LgWin& w, const uint16_t* __restrict__ hd, uint32_t* du,
                                                uint32_t* __restrict__ mxp, int H, int W, int wxe, int sx0) {
    constexpr int EH = E / 2, NG = E / 4, NR = VEC ? EH : E, PF = E <= 8 ? 8 : 64 / E;
    constexpr uint32_t HOUT = LG_HCAP;   // h outside the image: an upper bound that beats nothing
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int xl = sx0 + E * lane, xe = sx0 + 64 * E;   // the lane's first column, the span's end
    const int hx0 = (w.bx0 >> 6) << 6, hx1 = min(W, ((w.bx1 >> 6) + 1) << 6);   // columns lg_hrun_kernel wrote
    const int n = w.by1 - w.by0 + 1, na = n / 2;   // U is stored on rows [by0, by0 + na), D on the rows from there on
    const int dir = wave == 0 ? 1 : -1, ys = wave == 0 ? w.by0 : w.by1;
    const int cnt_a = wave == 0 ? na : n - na, cnt_b = n - cnt_a;
    // beside the span (sx0 % 4 == 0: the two columns left of it lie both in the image or both outside)
    const uint32_t fl = sx0 > 0 ? 0u : LG_INF, fr0 = xe < W ? 0u : LG_INF, fr1 = xe + 1 < W ? 0u : LG_INF;
    LgRowStep<E> rs;
    uint32_t mx = 0;
    auto load_h = [&](int y, uint32_t* raw) {   // raw words of row y: fix_h makes them h
        const uint16_t* row = hd + (size_t)y * W;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                const int xg = xl + 4 * g;
                const uint2 v = *reinterpret_cast<const uint2*>(row + ((xg >= hx0 && xg < hx1) ? xg : hx0));
                raw[2 * g] = v.x; raw[2 * g + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; k++) {
                const int c = xl + k;
                raw[k] = row[(c >= hx0 && c < hx1) ? c : hx0];
            }
        }
    };
    auto fix_h = [&](const uint32_t* raw, uint32_t* hp) {   // columns lg_hrun_kernel did not write: off the leaf, or outside the image
        if (VEC) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                const int xg = xl + 4 * g;
                const bool ld = xg >= hx0 && xg < hx1;
                const uint32_t f = xg < W ? 0u : (HOUT | (HOUT << 16));
                hp[2 * g] = ld ? raw[2 * g] : f; hp[2 * g + 1] = ld ? raw[2 * g + 1] : f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < EH; q++) {
                uint32_t hv[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int c = xl + 2 * q + k;
                    hv[k] = (c >= hx0 && c < hx1) ? raw[2 * q + k] : (c < W ? 0u : HOUT);
                }
                hp[q] = hv[0] | (hv[1] << 16);
            }
        }
    };
    // a parked row or a final one: the span's columns inside the window (wxe <= W; VEC: wxe % 4 == 0)
    auto load_row = [&](int y, uint32_t* raw) {   // columns that are not stored are not used either
        const uint32_t* row = du + (size_t)y * W;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                const int xg = xl + 4 * g;
                const uint4 v = *reinterpret_cast<const uint4*>(row + (xg < wxe ? xg : sx0));
                raw[4 * g] = v.x; raw[4 * g + 1] = v.y; raw[4 * g + 2] = v.z; raw[4 * g + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; k++) raw[k] = row[xl + k < wxe ? xl + k : sx0];
        }
    };
    auto store_row = [&](int y, const uint32_t* v) {
        uint32_t* row = du + (size_t)y * W;
        if (VEC) {
#pragma unroll
            for (int g = 0; g < NG; g++)
                if (xl + 4 * g < wxe) *reinterpret_cast<uint4*>(row + xl + 4 * g) = make_uint4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < E; k++)
                if (xl + k < wxe) row[xl + k] = v[k];
        }
    };
    auto edge_row = [&](int y, uint32_t* v) {   // a row beside the box
        const bool yin = y >= 0 && y < H;
#pragma unroll
        for (int k = 0; k < E; k++) v[k] = (yin && xl + k < W) ? 0u : LG_INF;
    };
    // cnt rows from row y0 on in the wave's direction; MEET: past mid-height
    auto run = [&](auto meet, int y0, int cnt) {
        constexpr bool MEET = decltype(meet)::value;
        uint32_t hq[PF][NR], oq[MEET ? PF : 1][MEET ? E : 1];
#pragma unroll
        for (int q = 0; q < PF; q++)
            if (q < cnt) {
                load_h(y0 + dir * q, hq[q]);
                if (MEET) load_row(y0 + dir * q, oq[q]);
            }
        for (int i0 = 0; i0 < cnt; i0 += PF) {
#pragma unroll
            for (int q = 0; q < PF; q++) {
                const int i = i0 + q;
                if (i < cnt) {   // (wave-uniform)
                    const int y = y0 + dir * i;
                    uint32_t hp[EH], v[E];
                    fix_h(hq[q], hp);
                    rs.step(hp, v, fl, fr0, fr1);
                    if (MEET) {
                        uint32_t o[E];
#pragma unroll
                        for (int k = 0; k < E; k++) {
                            const uint32_t d = min(v[k], oq[q][k]);
                            if (xl + k < wxe) mx = max(mx, d);
                            o[k] = __float_as_uint((float)d * (1.0f / 65536.0f));
                        }
                        store_row(y, o);
                    } else {
                        store_row(y, v);
                    }
                    if (i + PF < cnt) {
                        load_h(y + dir * PF, hq[q]);
                        if (MEET) load_row(y + dir * PF, oq[q]);
                    }
                }
            }
        }
    };
    if (wave < 2) {
        uint32_t v[E];
        const bool in2 = ys - 2 * dir >= 0 && ys - 2 * dir < H, in1 = ys - dir >= 0 && ys - dir < H;
        edge_row(ys - 2 * dir, v);
        rs.set_p2(v, in2 ? fl : LG_INF, in2 ? fr0 : LG_INF);
        edge_row(ys - dir, v);
        rs.set_p1(v, in1 ? fl : LG_INF, in1 ? fr0 : LG_INF, in1 ? fr1 : LG_INF);
        run(std::integral_constant<bool, false>(), ys, cnt_a);
    } else {
        // the rest of the window is off the leaf
        for (int y = w.wy0 + (wave - 2); y < w.wy1; y += 2) {
            const bool box_row = y >= w.by0 && y <= w.by1;
            uint32_t* row = du + (size_t)y * W;
            if (VEC) {
                for (int x = w.wx0 + 4 * lane; x < wxe; x += 256)
                    if (!(box_row && x >= sx0 && x < xe)) *reinterpret_cast<uint4*>(row + x) = make_uint4(0u, 0u, 0u, 0u);
            } else {
                for (int x = w.wx0 + lane; x < wxe; x += 64)
                    if (!(box_row && x >= sx0 && x < xe)) row[x] = 0u;
            }
        }
    }
    __syncthreads();   // (workgroup-scope release / acquire: the parked rows of the other wave)
    if (wave < 2) {
        run(std::integral_constant<bool, true>(), ys + dir * cnt_a, cnt_b);
        mx = lg_wave_max_u32(mx);
        if (lane == 0 && mx) atomicMax(mxp, mx);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void lg_dtsweep_kernel(const LgWin* __restrict__ wins, const uint32_t* __restrict__ tmp,
                                                         float* dist_out, uint32_t* __restrict__ maxfix, int H, int W, int wc) {
    const int frame = (int)blockIdx.x;   // (frame % 8 is the XCD whose L2 lg_hrun_kernel wrote the frame's run distances through)
    const LgWin w = wins[frame];
    if (!w.search_in) return;
    const int wxe = min(W, w.wx0 + w.nw * wc);
    const int sx0 = w.bx0 & ~3, span = w.bx1 - sx0 + 1;
    const uint16_t* hd = reinterpret_cast<const uint16_t*>(tmp + (size_t)frame * 2 * H * W);
    uint32_t* du = reinterpret_cast<uint32_t*>(dist_out + (size_t)frame * H * W);
    uint32_t* mxp = maxfix + frame * LG_MF;
    if (span <= 256) lg_dtsweep_body<4, VEC>(w, hd, du, mxp, H, W, wxe, sx0);
    else if (span <= 512) lg_dtsweep_body<8, VEC>(w, hd, du, mxp, H, W, wxe, sx0);
    else if (span <= 1024) lg_dtsweep_body<16, VEC>(w, hd, du, mxp, H, W, wxe, sx0);
    else lg_dtsweep_body<32, VEC>(w, hd, du, mxp, H, W, wxe, sx0);
}

static int lg_search_groups(int B, int per_batch, int lo, int hi) {
    const int bpad = 8 * ((B + 7) / 8);
    return std::max(lo, std::min(hi, per_batch / bpad));
}
// workgroups per frame of lg_dtband_kernel: four waves, each one band x one overlapping column tile at a time
static int lg_band_groups(int B, int H, int W, int P, int E) {
    const int S = 64 * E - 4 * (P - 2);
    const int units = ((W + S - 1) / S + 1) * ((H + P - 1) / P);
    return std::min((units + 3) / 4, lg_search_groups(B, 16384, 8, 512));
}
void lg_launch_hrun(const unsigned long long* bits, uint32_t* tmp, const LgWin* win, int B, int H, int W, int WW, hipStream_t s) {
    const int G = lg_search_groups(B, 2048, 2, 64);
    hipLaunchKernelGGL(lg_hrun_kernel, dim3(8u * G * ((B + 7) / 8)), dim3(256), 0, s, bits, win, tmp, H, W, WW, G, B);
}
// The row, seed and band kernels take the same arguments and the same grid: G workgroups per frame, dealt to the XCDs as
// lg_frame_of_block expects.
template <class K>
static void lg_launch_search(K kernel, int G, const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix,
                             const LgWin* win, int B, int H, int W, int WW, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3(8u * (unsigned)((B + 7) / 8) * G), dim3(256), 0, s, bits, win, tmp, dist_out, maxfix, H, W, WW,
                       lg_dt_geometry(W, nullptr), G, B);
}
// form 1: the one-level search of every row (one launch: small batches, where the launches' latency counts and the device is
// not full)
void lg_launch_dt_rows(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                       int H, int W, int WW, hipStream_t s) {
    lg_launch_search(lg_dtsearch_kernel, lg_search_groups(B, 8192, 8, 256), bits, tmp, dist_out, maxfix, win, B, H, W, WW, s);
}
// form 5: pairs of adjacent rows every band_p rows by the bounded search, then the rows between two pairs by the chamfer stencil
// run down and up in registers, band_e columns per lane.  Needs H, W >= 16 (the seed rows share the run distances' workspace).
template <class F>
static void lg_with_band_p(int band_p, F f) {   // f(std::integral_constant<int, P>) for the built P (16 for any other value)
    switch (band_p) {
        case 12: return f(std::integral_constant<int, 12>());
        case 24: return f(std::integral_constant<int, 24>());
        case 32: return f(std::integral_constant<int, 32>());
        default: return f(std::integral_constant<int, 16>());
    }
}
void lg_launch_dt_seeds(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, hipStream_t s) {
    lg_with_band_p(band_p, [&](auto p) {
        constexpr int P = decltype(p)::value;
        // workgroups per frame: the window's tiles (64 columns x 8 P rows) when the grid allows -- leaf tiles cluster, and a
        // workgroup that walks several of them with a fixed stride gets several heavy ones or none
        const int G = std::min((W + 63) / 64 * ((H + 8 * P - 1) / (8 * P)), lg_search_groups(B, 16384, 8, 512));
        lg_launch_search(lg_dtseed_kernel<P>, G, bits, tmp, dist_out, maxfix, win, B, H, W, WW, s);
    });
}
void lg_launch_dt_bands(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, int band_e, hipStream_t s) {
    const bool vec = W % band_e == 0;
    lg_with_band_p(band_p, [&](auto p) {
        constexpr int P = decltype(p)::value;
        auto go = [&](auto kernel, int E) {
            lg_launch_search(kernel, lg_band_groups(B, H, W, P, E), bits, tmp, dist_out, maxfix, win, B, H, W, WW, s);
        };
        if (band_e == 2) vec ? go(lg_dtband_kernel<P, 2, true>, 2) : go(lg_dtband_kernel<P, 2, false>, 2);
        else vec ? go(lg_dtband_kernel<P, 4, true>, 4) : go(lg_dtband_kernel<P, 4, false>, 4);
    });
}
// form 6 (W <= 2048: the span of any bounding box fits 64 lanes x 32 columns): one two-wave register sweep per frame
void lg_launch_dt_sweep(uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B, int H, int W, hipStream_t s) {
    const int wc = lg_dt_geometry(W, nullptr);
    if (W % 4 == 0) hipLaunchKernelGGL(lg_dtsweep_kernel<true>, dim3(B), dim3(256), 0, s, win, tmp, dist_out, maxfix, H, W, wc);
    else hipLaunchKernelGGL(lg_dtsweep_kernel<false>, dim3(B), dim3(256), 0, s, win, tmp, dist_out, maxfix, H, W, wc);
}
