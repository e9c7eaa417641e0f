// Leaf orientation on the device: GraspPointSelector.estimate_leaf_orientation
// (scripts/utils/grasp_point_selector.py:718-752) = cv2.findContours(RETR_EXTERNAL) -> max by cv2.contourArea ->
// cv2.minAreaRect -> direction of the longer side, per frame, from the bit rows of the mask's bounding box.
//
// One workgroup per frame, the same steps as the host analysis (lg_contour.cpp) and the same arithmetic:
//   A  runs of every bounding-box row (popcount of the run starts, workgroup prefix sum, extraction)
//   B  8-connected components of the runs: union-find in LDS (hook the larger root under the smaller with atomicMin; a
//      component's root is its first run in raster order = the start of its outer border)
//   C  more than one component: outer-border following per component (one lane each, Suzuki-Abe like the host), shoelace
//      sum in int64 (exact: the host's double sum never rounds either); largest area wins, first in raster order on ties
//   D  leftmost / rightmost pixel of the chosen component per row: only these can be hull vertices
//   E  strict vertices of the left (convex) and right (concave) chains by exact integer slope comparisons (in two levels: every
//      row against its block of 16 rows, then the blocks' vertices against each other), compacted in the order Andrew's
//      monotone chain produces (counter-clockwise from the lexicographically smallest point)
//   F  min-area rectangle over the hull edges in float64, no fused multiply-add (the host code has none): first minimum in
//      edge order, then atan2 / fmod, sin and cos for the score-plane kernel
// A frame with more runs than the scratch holds (or more hull vertices than LDS holds) gets status 1: the caller analyses
// that frame with the host code.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "lg_internal.h"
#include "lg_orient.h"

namespace {

typedef unsigned long long u64;
constexpr int OT = 256;     // threads per frame
constexpr int OHULL = 2048; // hull vertices held in LDS (a convex lattice polygon in a 16384-box has < 2300 / 2 of them)

struct Band { const u64* rows; int hy, W, WW, w0, w1; };   // rows -> image row by0; only words [w0, w1] hold leaf pixels

__device__ __forceinline__ u64 band_word(const Band& bd, int y, int w) {
    u64 v = (y < 0 || y >= bd.hy || w < bd.w0 || w > bd.w1) ? 0ull : bd.rows[(size_t)y * bd.WW + w];
    if (w == bd.WW - 1 && (bd.W & 63)) v &= (~0ull) >> (64 - (bd.W & 63));
    return v;
}

// pixels x-1, x, x+1 of band row y in bits 0..2
__device__ __forceinline__ unsigned row3(const Band& bd, int y, int x) {
    if (y < 0 || y >= bd.hy) return 0;
    const int xa = x - 1, xb = x + 1;
    const int wa = xa >> 6, wb = xb >> 6, wm = x >> 6;   // xa = -1 -> word -1: outside
    const u64 lo = band_word(bd, y, wa);
    const u64 hi = wb == wa ? lo : band_word(bd, y, wb);
    unsigned r = 0;
    if (xa >= 0) r |= (unsigned)((lo >> (xa & 63)) & 1ull);
    r |= (unsigned)((((wm == wa) ? lo : hi) >> (x & 63)) & 1ull) << 1;
    if (xb < bd.W) r |= (unsigned)((hi >> (xb & 63)) & 1ull) << 2;
    return r;
}

// neighbours of (x, y), bit d = direction d: clockwise on the screen starting at West (W NW N NE E SE S SW), lg_contour.cpp
__device__ __forceinline__ unsigned ring_at(const Band& bd, int x, int y) {
    const unsigned up = row3(bd, y - 1, x), mid = row3(bd, y, x), dn = row3(bd, y + 1, x);
    return (mid & 1u) | ((up & 1u) << 1) | (((up >> 1) & 1u) << 2) | (((up >> 2) & 1u) << 3) | (((mid >> 2) & 1u) << 4) |
           (((dn >> 2) & 1u) << 5) | (((dn >> 1) & 1u) << 6) | ((dn & 1u) << 7);
}
__device__ __forceinline__ int dir_dx(int d) { return (int)((0x1A90u >> (2 * d)) & 3u) - 1; }   // -1 -1 0 1 1 1 0 -1
__device__ __forceinline__ int dir_dy(int d) { return (int)((0xA901u >> (2 * d)) & 3u) - 1; }   //  0 -1 -1 -1 0 1 1 1

// twice the shoelace area of the outer border that starts at (sx, sy), the top-most / left-most pixel of its component
__device__ long long trace_area2(const Band& bd, int sx, int sy) {
    unsigned ring = ring_at(bd, sx, sy);
    if (!ring) return 0;                                 // single pixel
    const int first = __builtin_ctz(ring);               // first neighbour clockwise from West
    const int fx = sx + dir_dx(first), fy = sy + dir_dy(first);
    int cx = sx, cy = sy, dprev = first, lastx = 0, lasty = 0;
    bool have_last = false;
    long long acc = 0, guard = 8ll * ((long long)bd.hy * bd.W + 16);
    for (;;) {
        // counter-clockwise from the previous pixel: directions dprev-1, dprev-2, ... = bits 7, 6, ... of the rotated ring
        const unsigned r = ((ring >> dprev) | (ring << (8 - dprev))) & 0xffu;
        if (have_last) acc += (long long)lastx * cy - (long long)cx * lasty;
        lastx = cx; lasty = cy; have_last = true;
        if (!r) break;
        const int m = 31 - __builtin_clz(r);
        const int d = (dprev - (8 - m)) & 7;
        const int nx = cx + dir_dx(d), ny = cy + dir_dy(d);
        if (nx == sx && ny == sy && cx == fx && cy == fy) break;
        cx = nx; cy = ny; dprev = (d + 4) & 7;
        ring = ring_at(bd, cx, cy);
        if (--guard < 0) break;
    }
    acc += (long long)lastx * sy - (long long)sx * lasty;
    return acc < 0 ? -acc : acc;
}

// exclusive prefix sum of one int per thread; total to every thread
__device__ int block_scan(int v, int* s, int* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < OT; d <<= 1) {
        const int a = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[OT - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ int uf_find(int* p, int i) {
    int r;
    while ((r = __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != i) i = r;
    return i;
}
__device__ void uf_union(int* p, int a, int b) {
    for (;;) {
        a = uf_find(p, a);
        b = uf_find(p, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(p + b, a);   // b was a root: hook it under the smaller root
        if (old == b) return;
        b = old;                               // somebody hooked b meanwhile: (a, old) still have to meet
    }
}

struct FrameScratch {
    uint32_t* run_x;   // x0 | x1 << 16
    uint16_t* run_y;   // row inside the band
    int* roots;
    int* row_start;    // [hy + 1]
    short* rowL;       // leftmost / rightmost pixel of the chosen component per band row (-1: none)
    short* rowR;
    unsigned char* vflag;   // [2][hy] strict hull vertex on the left / right chain
    int* comp;              // [4][cap] per component (indexed by its root run): interior pixels, min x, max x, last row
};

// -DLG_ORIENT_PHASES (off in the shipped build; LG_VARIANT_SRC=lg_orient.hip tools/build_variants.sh "phases:-DLG_ORIENT_PHASES"):
// thread 0 of the first OPH_FRAMES frames of a launch stamps wall_clock64() (100 MHz) at the kernel's start, behind the steps A, B,
// C, D, E, behind the compaction and at the end; lg_debug_orient_phases reads the stamps (tools/orient_phases.py prints them)
#ifdef LG_ORIENT_PHASES
constexpr int OPH_FRAMES = 256, OPH_N = 8;
__device__ unsigned long long lg_orient_phase_clk[OPH_FRAMES * OPH_N];
#define OPHASE(k) do { if (tid == 0 && b < OPH_FRAMES) lg_orient_phase_clk[b * OPH_N + (k)] = wall_clock64(); } while (0)
#else
#define OPHASE(k) do { } while (0)
#endif

constexpr int OBLK = 16;   // rows per block of step E's first level (a power of two, at most 64)

// Step E's vertex test on the rows row(ja) < ... < row(jb - 1): is row(j) a strict vertex of their left chain (LEFT: lower
// convex envelope of X over the rows -- the steepest slope arriving from above is smaller than the flattest slope leaving
// downwards) or of their right chain (mirrored)?  The first and the last row always are.  Exact integer comparisons.
template <bool LEFT, class RowOf>
__device__ __forceinline__ bool hull_vertex(const short* X, RowOf row, int ja, int j, int jb) {
    if (j == ja || j == jb - 1) return true;
    const int i = row(j), xi = X[i], ra = row(ja), rb = row(j + 1);
    int p = xi - X[ra], q = i - ra;                      // arriving slopes (x_i - x_a) / (i - a): max (left), min (right)
    for (int a = ja + 1; a < j; a++) {
        const int r = row(a), qq = i - r, pp = xi - X[r];
        if (LEFT ? pp * q > p * qq : pp * q < p * qq) { p = pp; q = qq; }
    }
    int p2 = X[rb] - xi, q2 = rb - i;                    // leaving slopes (x_b - x_i) / (b - i): min (left), max (right)
    for (int c = j + 2; c < jb; c++) {
        const int r = row(c), qq = r - i, pp = X[r] - xi;
        if (LEFT ? pp * q2 < p2 * qq : pp * q2 > p2 * qq) { p2 = pp; q2 = qq; }
    }
    return LEFT ? p * q2 < p2 * q : p * q2 > p2 * q;
}

// A frame's parameters and status word: into device memory (the plane kernel reads fp) and, where the host's pinned copies
// have device aliases (fp_h, status_h: both or neither), straight into those -- the host reads them behind the event it waits
// for, without a copy in between.
struct OrientOut {
    LgFrameParams* fp;
    int* status;
    LgFrameParams* fp_h;
    int* status_h;
};
__device__ __forceinline__ void put_frame(const OrientOut& o, int b, const LgFrameParams& f, int st) {
    o.fp[b] = f;
    o.status[b] = st;
    if (o.fp_h) { o.fp_h[b] = f; o.status_h[b] = st; }
}

__device__ void write_none(const OrientOut& o, double* out, int b, int st) {
    LgFrameParams f;
    f.sin_t = 0.f; f.cos_t = 0.f; f.has_angle = 0; f.theta = __builtin_nanf("");
    for (int i = 0; i < 5; i++) out[5 * (size_t)b + i] = __builtin_nan("");
    put_frame(o, b, f, st);
}

__global__ __launch_bounds__(OT) void lg_orient_kernel(const u64* __restrict__ bits, const LgWin* __restrict__ win, int H, int W,
                                                       int WW, int cap, uint32_t* run_x_, uint16_t* run_y_, int* roots_,
                                                       int* row_start_, short* rowL_, short* rowR_, unsigned char* vflag_,
                                                       int* comp_, OrientOut oo, double* out) {
#pragma clang fp contract(off)
    // parent[cap] | L[n], R[n] shorts, survivor lists [n], [n], ballots | hull x[OHULL], y[OHULL] doubles
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ int s_scan[OT];
    __shared__ int s_nroots, s_ybot, s_rank, s_lb, s_ncand, s_cand;
    __shared__ u64 s_key, s_p0;
    const int b = blockIdx.x, tid = threadIdx.x;
    const LgWin w = win[b];
    const int hyb = w.by1 - w.by0 + 1;
    if (w.bx1 < w.bx0 || hyb <= 0) {                      // empty mask: the reference returns None
        if (tid == 0) write_none(oo, out, b, 0);
        return;
    }
    FrameScratch fs;
    fs.run_x = run_x_ + (size_t)b * cap; fs.run_y = run_y_ + (size_t)b * cap; fs.roots = roots_ + (size_t)b * cap;
    fs.row_start = row_start_ + (size_t)b * (H + 1); fs.rowL = rowL_ + (size_t)b * H; fs.rowR = rowR_ + (size_t)b * H;
    fs.vflag = vflag_ + (size_t)b * 2 * H;
    fs.comp = comp_ + (size_t)b * 4 * cap;
    Band bd;
    bd.rows = bits + ((size_t)b * H + w.by0) * WW; bd.hy = hyb; bd.W = W; bd.WW = WW; bd.w0 = w.bx0 >> 6; bd.w1 = w.bx1 >> 6;
    if (tid == 0) { s_nroots = 0; s_ybot = 0; s_key = 0; s_p0 = ~0ull; s_rank = 0x7fffffff; s_lb = 0; s_ncand = 0; s_cand = 0; }
    OPHASE(0);
    // ---- A: runs.  Thread t owns the rows [r0, r1)
    const int chunk = (hyb + OT - 1) / OT, r0 = min(tid * chunk, hyb), r1 = min(r0 + chunk, hyb);
    int sum = 0;
    for (int r = r0; r < r1; r++) {
        int cnt = 0;
        u64 in = 0;
        for (int q = bd.w0; q <= bd.w1; q++) {
            const u64 v = band_word(bd, r, q);
            cnt += __popcll(v & ~((v << 1) | in));
            in = v >> 63;
        }
        fs.row_start[r] = cnt;
        sum += cnt;
    }
    int R = 0;
    int base = block_scan(sum, s_scan, &R);
    if (R > cap) {
        if (tid == 0) write_none(oo, out, b, 1);
        return;
    }
    int* parent = (int*)s_dyn;
    for (int r = r0; r < r1; r++) {
        const int cnt = fs.row_start[r];
        fs.row_start[r] = base;
        int idx = base, start = 0;
        base += cnt;
        u64 in = 0;
        for (int q = bd.w0; q <= bd.w1; q++) {
            const u64 v = band_word(bd, r, q);
            u64 tr = v ^ ((v << 1) | in);               // bit k: pixel k differs from pixel k-1
            bool inside = in != 0;
            while (tr) {
                const int x = q * 64 + __builtin_ctzll(tr);
                tr &= tr - 1;
                if (!inside) { inside = true; start = x; }
                else {
                    inside = false;
                    fs.run_x[idx] = (uint32_t)start | ((uint32_t)(x - 1) << 16);
                    fs.run_y[idx] = (uint16_t)r;
                    parent[idx] = idx;
                    idx++;
                }
            }
            in = v >> 63;
        }
        if (in) {
            fs.run_x[idx] = (uint32_t)start | ((uint32_t)min(W - 1, 64 * (bd.w1 + 1) - 1) << 16);
            fs.run_y[idx] = (uint16_t)r;
            parent[idx] = idx;
        }
    }
    if (tid == 0) fs.row_start[hyb] = R;
    __syncthreads();
    OPHASE(1);
    // ---- B: union runs that touch the previous row (8-connectivity: overlap after growing by one pixel)
    for (int i = tid; i < R; i += OT) {
        const int r = fs.run_y[i];
        if (r == 0) continue;
        const uint32_t xi = fs.run_x[i];
        const int x0 = (int)(xi & 0xffffu), x1 = (int)(xi >> 16);
        int lo = fs.row_start[r - 1];
        const int hi = fs.row_start[r];
        int l = lo, h = hi;                              // first run a of the previous row with x1a + 1 >= x0
        while (l < h) {
            const int m = (l + h) >> 1;
            if ((int)(fs.run_x[m] >> 16) + 1 >= x0) h = m; else l = m + 1;
        }
        for (int a = l; a < hi; a++) {
            if ((int)(fs.run_x[a] & 0xffffu) > x1 + 1) break;
            uf_union(parent, a, i);
        }
    }
    __syncthreads();
    for (int i = tid; i < R; i += OT) {
        const int root = uf_find(parent, i);
        if (root == i) {
            fs.roots[atomicAdd(&s_nroots, 1)] = i;
            fs.comp[i] = 0; fs.comp[cap + i] = 0x7fffffff; fs.comp[2 * cap + i] = -1; fs.comp[3 * cap + i] = -1;
        }
    }
    __syncthreads();
    for (int i = tid; i < R; i += OT) parent[i] = uf_find(parent, i);   // (a root stays a root: concurrent reads still end there)
    const int nroots = s_nroots;
    __syncthreads();
    OPHASE(2);
    // ---- C: the component with the largest outer contour
    int best;
    if (nroots == 1) {
        best = fs.roots[0];
    } else {
        // Which components can hold the largest outer contour at all?  Following a border is serial (one lane per component, a
        // dependent chain of bit-row loads per step: ~1 us per border pixel), so a leaf with a few specks beside it would cost a
        // few thousand steps for a decision that is obvious.  Two bounds on a component's contour area A (the area of the polygon
        // through the centres of its outer border pixels): A >= the number of its pixels whose whole 3 x 3 neighbourhood is set
        // (their unit squares are disjoint and lie inside that polygon) and A <= (width - 1) (height - 1) of its bounding box.
        // A component whose upper bound is below the best lower bound is out -- it cannot even tie.  One survivor: no border is
        // followed at all.
        for (int i = tid; i < R; i += OT) {
            const int root = parent[i], r = fs.run_y[i];
            const uint32_t xi = fs.run_x[i];
            const int x0 = (int)(xi & 0xffffu), x1 = (int)(xi >> 16);
            int inner = 0;
            if (x1 - x0 >= 2 && r > 0 && r < hyb - 1) {
                for (int q = x0 >> 6; q <= (x1 >> 6); q++) {
                    const u64 f0 = band_word(bd, r - 1, q - 1) & band_word(bd, r, q - 1) & band_word(bd, r + 1, q - 1);
                    const u64 f1 = band_word(bd, r - 1, q) & band_word(bd, r, q) & band_word(bd, r + 1, q);
                    const u64 f2 = band_word(bd, r - 1, q + 1) & band_word(bd, r, q + 1) & band_word(bd, r + 1, q + 1);
                    u64 in3 = f1 & ((f1 << 1) | (f0 >> 63)) & ((f1 >> 1) | (f2 << 63));
                    const int lo = max(x0 - q * 64, 0), hi = min(x1 - q * 64, 63);
                    in3 &= (~0ull << lo) & (~0ull >> (63 - hi));
                    inner += __popcll(in3);
                }
            }
            if (inner) atomicAdd(&fs.comp[root], inner);
            atomicMin(&fs.comp[cap + root], x0);
            atomicMax(&fs.comp[2 * cap + root], x1);
            atomicMax(&fs.comp[3 * cap + root], r);
        }
        __threadfence_block();
        __syncthreads();
        for (int k = tid; k < nroots; k += OT) atomicMax(&s_lb, fs.comp[fs.roots[k]]);
        __syncthreads();
        const long long lb2 = 2ll * s_lb;
        for (int k = tid; k < nroots; k += OT) {
            const int root = fs.roots[k];
            const long long ub2 = 2ll * (fs.comp[2 * cap + root] - fs.comp[cap + root]) * (fs.comp[3 * cap + root] - (int)fs.run_y[root]);
            if (ub2 >= lb2) { atomicAdd(&s_ncand, 1); atomicMax(&s_cand, root); } else fs.roots[k] = -1;
        }
        __syncthreads();
        if (s_ncand == 1) {
            if (tid == 0) s_key = (u64)(0xfffff - s_cand);
        } else {
            for (int k = tid; k < nroots; k += OT) {
                const int root = fs.roots[k];
                if (root < 0) continue;
                const long long a2 = trace_area2(bd, (int)(fs.run_x[root] & 0xffffu), (int)fs.run_y[root]);
                atomicMax(&s_key, ((u64)a2 << 20) | (u64)(0xfffff - root));   // a2 <= 2 H W < 2^29; equal areas: first in raster order
            }
        }
        __syncthreads();
        best = 0xfffff - (int)(s_key & 0xfffffull);
    }
    OPHASE(3);
    // ---- D: per row, leftmost / rightmost pixel of that component
    for (int r = r0; r < r1; r++) {
        int L = -1, Rr = -1;
        for (int i = fs.row_start[r]; i < fs.row_start[r + 1]; i++)
            if (parent[i] == best) {
                const uint32_t xi = fs.run_x[i];
                if (L < 0) L = (int)(xi & 0xffffu);
                Rr = (int)(xi >> 16);
            }
        fs.rowL[r] = (short)L; fs.rowR[r] = (short)Rr;
        if (L >= 0) atomicMax(&s_ybot, r);
    }
    __syncthreads();                                      // parent[] is dead from here on
    const int ytop = fs.run_y[best], n = s_ybot - ytop + 1;   // a component covers a contiguous range of rows
    short* Ls = (short*)s_dyn;
    short* Rs = Ls + n;
    for (int i = tid; i < n; i += OT) { Ls[i] = fs.rowL[ytop + i]; Rs[i] = fs.rowR[ytop + i]; }
    __syncthreads();
    OPHASE(4);
    // ---- E: strict hull vertices.  Left chain = lower convex envelope of L over the rows: row i is a vertex iff the
    // steepest slope arriving from above is smaller than the flattest slope leaving downwards; right chain mirrored.
    // In two levels: a strict vertex of the hull of all rows is a strict vertex of the hull of any subset that holds it, and the
    // hull of all rows is the hull of the subsets' vertices.  Level 1 tests every row against the rows of its own block of
    // OBLK; level 2 tests the survivors of a chain against each other -- the same integer comparisons on fewer rows.
    uint16_t* listL = (uint16_t*)(Rs + n);                // level-1 survivors of the two chains, ascending rows
    uint16_t* listR = listL + n;
    u64* mskL = (u64*)(s_dyn + 8 * (size_t)n);            // their ballots per 64 rows
    const int nseg = (n + 63) >> 6;
    u64* mskR = mskL + nseg;
    const auto same = [](int j) { return j; };
    for (int base = 0; base < n; base += OT) {            // (every lane of a wave takes part in the ballots)
        const int i = base + tid;
        bool vl = false, vr = false;
        if (i < n) {
            const int b0 = i & ~(OBLK - 1), b1 = min(b0 + OBLK, n);
            vl = hull_vertex<true>(Ls, same, b0, i, b1);
            vr = hull_vertex<false>(Rs, same, b0, i, b1);
            if (!vl) fs.vflag[i] = 0;
            if (!vr) fs.vflag[H + i] = 0;
        }
        const u64 ml = __ballot(vl), mr = __ballot(vr);
        if ((tid & 63) == 0 && i < n) { mskL[i >> 6] = ml; mskR[i >> 6] = mr; }
    }
    __syncthreads();
    int SL = 0, SR = 0, sdone = 0;                        // survivors in the 64-row segments [0, sdone)
    for (int base = 0; base < n; base += OT) {
        const int i = base + tid, seg = i >> 6, lane = tid & 63;
        if (seg >= nseg) break;
        for (; sdone < seg; sdone++) { SL += __popcll(mskL[sdone]); SR += __popcll(mskR[sdone]); }
        const u64 ml = mskL[seg], mr = mskR[seg], below = (1ull << lane) - 1ull;
        if ((ml >> lane) & 1ull) listL[SL + __popcll(ml & below)] = (uint16_t)i;
        if ((mr >> lane) & 1ull) listR[SR + __popcll(mr & below)] = (uint16_t)i;
    }
    for (; sdone < nseg; sdone++) { SL += __popcll(mskL[sdone]); SR += __popcll(mskR[sdone]); }
    __syncthreads();
    for (int it = tid; it < SL + SR; it += OT) {
        if (it < SL) {
            fs.vflag[listL[it]] = hull_vertex<true>(Ls, [listL](int j) { return (int)listL[j]; }, 0, it, SL);
        } else {
            const int k = it - SL, i = listR[k];
            bool vr = hull_vertex<false>(Rs, [listR](int j) { return (int)listR[j]; }, 0, k, SR);
            // the chains meet at the top and bottom rows: a shared end point is listed once (with the left chain)
            if ((i == 0 || i == n - 1) && Ls[i] == Rs[i]) vr = false;
            fs.vflag[H + i] = vr;
        }
    }
    __syncthreads();
    OPHASE(5);
    // order: left chain bottom -> top, then right chain top -> bottom (Andrew's monotone chain on (x, y) walks the hull
    // this way round); the start at the lexicographically smallest point is applied as a rotation below
    const int chn = (n + OT - 1) / OT, i0 = min(tid * chn, n), i1 = min(i0 + chn, n);
    int cl = 0, cr = 0;
    for (int i = i0; i < i1; i++) { cl += fs.vflag[i]; cr += fs.vflag[H + i]; }
    int totL = 0, totR = 0;
    int bl = block_scan(cl, s_scan, &totL);
    int br = block_scan(cr, s_scan, &totR);
    const int nh = totL + totR;
    if (nh > OHULL) {
        if (tid == 0) write_none(oo, out, b, 1);
        return;
    }
    double* hx = (double*)s_dyn;                          // (Ls / Rs are dead: every thread passed the scans' barriers)
    double* hyv = hx + OHULL;
    for (int i = i0; i < i1; i++) {
        const int yabs = w.by0 + ytop + i;
        if (fs.vflag[i]) {
            const int pos = totL - 1 - bl;
            bl++;
            const int x = fs.rowL[ytop + i];
            hx[pos] = (double)x; hyv[pos] = (double)yabs;
            atomicMin(&s_p0, ((u64)x << 32) | ((u64)yabs << 16) | (u64)pos);
        }
        if (fs.vflag[H + i]) {
            const int pos = totL + br;
            br++;
            hx[pos] = (double)fs.rowR[ytop + i]; hyv[pos] = (double)yabs;   // (never the smallest point: the left chain holds it)
        }
    }
    __syncthreads();
    if (nh == 1) {
        if (tid == 0) {
            LgFrameParams f;
            const double ang = M_PI / 2;
            f.sin_t = (float)sin(ang); f.cos_t = (float)cos(ang); f.has_angle = 1; f.theta = (float)ang;
            double* o = out + 5 * (size_t)b;
            o[0] = ang; o[1] = 0; o[2] = 0; o[3] = hx[0]; o[4] = hyv[0];
            put_frame(oo, b, f, 0);
        }
        return;
    }
    OPHASE(6);
    // ---- F: min-area rectangle, one hull edge per thread (edge e starts at hull vertex e counted from the smallest point)
    const int pos0 = (int)(s_p0 & 0xffffull);
    double m_area = 1e300, m_ux = 0, m_uy = 0, m_w = 0, m_h = 0, m_sc = 0, m_tc = 0;
    int m_rank = 0x7fffffff;
    const int nedges = nh == 2 ? 1 : nh;
    for (int e = tid; e < nedges; e += OT) {
        int i = pos0 + e;
        if (i >= nh) i -= nh;
        const int i2 = i + 1 >= nh ? i + 1 - nh : i + 1;
        const double ex = hx[i2] - hx[i], ey = hyv[i2] - hyv[i], len = sqrt(ex * ex + ey * ey);
        if (len == 0) continue;
        const double ux = ex / len, uy = ey / len;
        double smin = 1e300, smax = -1e300, tmin = 1e300, tmax = -1e300;
        int j = pos0;
        for (int c = 0; c < nh; c++) {
            const double px = hx[j], py = hyv[j];
            const double s = px * ux + py * uy;
            const double t = -px * uy + py * ux;
            smin = s < smin ? s : smin; smax = s > smax ? s : smax;
            tmin = t < tmin ? t : tmin; tmax = t > tmax ? t : tmax;
            if (++j >= nh) j = 0;
        }
        const double area = (smax - smin) * (tmax - tmin);
        if (area < m_area) {
            m_area = area; m_rank = e; m_ux = ux; m_uy = uy;
            m_w = smax - smin; m_h = tmax - tmin;
            m_sc = 0.5 * (smin + smax); m_tc = 0.5 * (tmin + tmax);
        }
    }
    if (tid == 0) s_key = ~0ull;
    __syncthreads();
    if (m_rank != 0x7fffffff) atomicMin(&s_key, (u64)__double_as_longlong(m_area));   // areas are >= 0: bit order = value order
    __syncthreads();
    if (m_rank != 0x7fffffff && (u64)__double_as_longlong(m_area) == s_key) atomicMin(&s_rank, m_rank);
    __syncthreads();
    if (s_rank == 0x7fffffff) {                            // (cannot happen: distinct vertices give edges of non-zero length)
        if (tid == 0) write_none(oo, out, b, 1);
        return;
    }
    if (m_rank == s_rank) {
        const double bang = atan2(m_uy, m_ux);
        double ang = (m_w < m_h) ? bang + M_PI / 2 : bang;
        ang = fmod(ang, M_PI);
        if (ang <= 0) ang += M_PI;
        LgFrameParams f;
        f.sin_t = (float)sin(ang); f.cos_t = (float)cos(ang); f.has_angle = 1; f.theta = (float)ang;
        double* o = out + 5 * (size_t)b;
        o[0] = ang; o[1] = m_w > m_h ? m_w : m_h; o[2] = m_w < m_h ? m_w : m_h;
        o[3] = m_sc * m_ux - m_tc * m_uy; o[4] = m_sc * m_uy + m_tc * m_ux;
        put_frame(oo, b, f, 0);
    }
    OPHASE(7);
}

template <typename T>
hipError_t dalloc(T** p, size_t n) { return hipMalloc((void**)p, n * sizeof(T)); }

}  // namespace

#ifdef LG_ORIENT_PHASES
// out[frame][8]: the stamps of the last launch's first `frames` frames (synchronise the launch's stream first)
extern "C" int lg_debug_orient_phases(unsigned long long* out, int frames) {
    if (!out || frames < 1 || frames > OPH_FRAMES) return LG_ERR_INVALID;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(lg_orient_phase_clk), sizeof(unsigned long long) * OPH_N * frames) == hipSuccess
               ? LG_OK : LG_ERR_HIP;
}
#endif

void lg_orient_free(LgOrientWs*& w) {
    if (!w) return;
    hipFree(w->run_x); hipFree(w->run_y); hipFree(w->roots); hipFree(w->row_start); hipFree(w->rowL); hipFree(w->rowR);
    hipFree(w->vflag); hipFree(w->comp); hipFree(w->out); hipFree(w->status);
    if (w->h_out) hipHostFree(w->h_out);
    if (w->h_status) hipHostFree(w->h_status);
    delete w;
    w = nullptr;
}

int lg_orient_ensure(LgOrientWs*& w, int B, int H, int cap, std::string* err) {
    if (w && B <= w->capB && H == w->H) return LG_OK;
    const int nB = std::max(B, w ? w->capB : 0);
    hipDeviceSynchronize();
    lg_orient_free(w);
    w = new LgOrientWs();
    w->cap = cap;
    const size_t nb = (size_t)nB;
    hipError_t rc = hipSuccess;
    auto A = [&](hipError_t r) { if (rc == hipSuccess) rc = r; };
    A(dalloc(&w->run_x, nb * w->cap)); A(dalloc(&w->run_y, nb * w->cap)); A(dalloc(&w->roots, nb * w->cap));
    A(dalloc(&w->row_start, nb * (H + 1))); A(dalloc(&w->rowL, nb * H)); A(dalloc(&w->rowR, nb * H));
    A(dalloc(&w->vflag, nb * 2 * H)); A(dalloc(&w->comp, nb * 4 * w->cap)); A(dalloc(&w->out, nb * 5)); A(dalloc(&w->status, nb));
    A(hipHostMalloc((void**)&w->h_out, sizeof(double) * 5 * nb));
    A(hipHostMalloc((void**)&w->h_status, sizeof(int) * nb));
    // device-side alias of the pinned status words (lg_launch_orient with fp_host_dev writes them directly); none: copies
    if (rc == hipSuccess && hipHostGetDevicePointer((void**)&w->h_status_dev, w->h_status, 0) != hipSuccess) {
        w->h_status_dev = nullptr;
        (void)hipGetLastError();
    }
    if (rc != hipSuccess) {
        if (err) *err = std::string("orientation scratch: ") + hipGetErrorString(rc);
        lg_orient_free(w);
        return LG_ERR_NOMEM;
    }
    w->capB = nB; w->H = H;
    // LDS: parent[cap] ints; later step E's two short rows [H], two survivor lists [H] and two ballots per 64 rows; then the
    // hull (2 * OHULL doubles)
    w->lds = std::max(std::max((size_t)w->cap * 4, (size_t)H * 8 + ((size_t)H / 64 + 1) * 16), (size_t)OHULL * 16);
    rc = hipFuncSetAttribute((const void*)lg_orient_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w->lds);
    if (rc != hipSuccess) {
        if (err) *err = std::string("orientation kernel LDS: ") + hipGetErrorString(rc);
        lg_orient_free(w);
        return LG_ERR_HIP;
    }
    return LG_OK;
}

// frames [off, off + n) of the workspace: bits / win / fp point at frame `off`
void lg_launch_orient(LgOrientWs* w, const unsigned long long* bits, const LgWin* win, LgFrameParams* fp, int off, int n, int H,
                      int W, int WW, hipStream_t s, LgFrameParams* fp_host_dev) {
    const size_t o = (size_t)off;
    OrientOut oo;
    oo.fp = fp; oo.status = w->status + o;
    const bool direct = fp_host_dev && w->h_status_dev;
    oo.fp_h = direct ? fp_host_dev : nullptr;
    oo.status_h = direct ? w->h_status_dev + o : nullptr;
    hipLaunchKernelGGL(lg_orient_kernel, dim3(n), dim3(OT), w->lds, s, bits, win, H, W, WW, w->cap, w->run_x + o * w->cap,
                       w->run_y + o * w->cap, w->roots + o * w->cap, w->row_start + o * (H + 1), w->rowL + o * H, w->rowR + o * H,
                       w->vflag + o * 2 * H, w->comp + o * 4 * w->cap, oo, w->out + 5 * o);
}
