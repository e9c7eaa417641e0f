// The fused score-plane kernel with its launch forms, the near-tile enumeration in front of it, and smooth_depth on its own.
// Reference semantics: scripts/utils/grasp_point_selector.py (cited per kernel); design: DESIGN.md.
#include "lg_planes.h"
#include "lg_pixel.h"
#include "lg_wave.h"

#include <hip/hip_ext.h>

#include <algorithm>

// ============================================================================ fused score planes
// One pass producing sdf_score, approach, flatness, isolation, accessibility, stem, traditional and the
// validity mask (grasp_point_selector.py:256-288) from depth + mask bits + distance_map (+ frame scalars).
// Tile 64 x LG_TH (16), 256 threads, each thread 4 consecutive pixels x LG_TH/16 rows (16-byte stores per lane).
//
// Launch shape: one workgroup per tile, or (LG_FINAL_PERSIST, lg_launch_final) resident workgroups that walk the tiles, or (near
// launch, sparse mode) one workgroup per entry of the batch's list of near tiles; the same code serves all -- blockIdx % 8 is the XCD, every XCD owns a contiguous range of tiles and its workgroups take them
// with the XCD's workgroup count as stride, so neighbouring workgroups work on neighbouring tiles at the same time (shared
// halos hit in the XCD's L2).
// What the tile loop needs from the code: nothing loop-invariant may stay in registers across tiles at 64 VGPRs (8 waves per
// SIMD; 66 gave 7) -- the arguments are read through the kernarg pointer, laundered once per tile (their ~60 scalar loads then
// belong to the iteration instead of being hoisted: without this 156 SGPRs + 39 VGPRs spilled), the thread index likewise
// (indices and LDS addresses are recomputed per tile), the tile walk is 32-bit scalar arithmetic, frame scalars come
// through the scalar cache, and the barriers order LDS only (s_waitcnt lgkmcnt(0)): __syncthreads() would also wait for the
// previous tile's plane stores to be acknowledged.
// What bounds it (tools/ubench/stream_mix.hip, tools/final_ablate.sh, one box): a kernel with ONLY this path's loads and
// stores in the same 64 x 16 tile shape reaches 0.72 of the 8 TB/s peak (1.70 ms per 128 frames; a plain 2-read + 1-write copy
// 0.65, the nine stores alone 0.84, 256 x 4 tiles 0.82); this kernel with its arithmetic removed 1.98 ms, complete 2.21 ms.
// Occupancy: the stencil path scales with the waves in flight -- every tile on the stencil path, 128 frames of 1080p, one
// workgroup per tile: 3.23 / 2.80 / 2.63 / 2.37 ms at 4 / 5 / 6-7 / 8 waves per SIMD (tools/final_dense.py).
#ifndef LG_FINAL_WPE
#define LG_FINAL_WPE 8
#endif
#define LG_FINAL_WPE_ATTR __attribute__((amdgpu_waves_per_eu(LG_FINAL_WPE, LG_FINAL_WPE)))
// VEC: W % 4 == 0 (16-byte loads / stores everywhere); ALL: every plane and the validity plane are wanted (the dense
// call with the CNN): the instantiation for the usual case carries no per-plane null checks and no scalar store paths.
// SCORE (deferred planes, LgFinalArgs::score_only; with ALL = false): what top-k reads is stored -- traditional, validity --,
// distance = 0 outside the sweep window, which the gather still reads, and flatness (see lg_tap_row), again without null
// checks; sdf, approach, isolation, accessibility and stem are not stored and the isolation arithmetic is not done:
// lg_gather_kernel computes those five at its windows.
// R: radius of the separable Gaussian of ImageProcessor.smooth_depth (gaussian_size = 2R+1: 1, 3, 5 = the node's, 7); the
// stencil reaches HALO = R + 1 pixels (Gaussian, then the 3x3 Sobel).
template <bool VEC, bool ALL, int R, bool SCORE = false>
__global__ __launch_bounds__(256) LG_FINAL_WPE_ATTR void lg_final_kernel(LgFinalArgs a_) {
    static_assert(!(ALL && SCORE), "score-only stores fewer planes than ALL");
    constexpr int HALO = R + 1;
    static_assert(R >= 0 && HALO <= 4, "the depth tile carries 4 halo columns");
    constexpr int DW = 72;             // dm tile: cols tx0-4 .. tx0+67
    constexpr int DH = LG_TH + 2 * HALO;   // rows ty0-HALO .. ty0+LG_TH-1+HALO
    constexpr int GW = LG_TW + 2;      // g tile: cols tx0-1 .. tx0+64
    constexpr int GH = LG_TH + 2;
    __shared__ __attribute__((aligned(16))) float s_dm[DH * DW];
    __shared__ float s_h[DH * GW];
    float* const s_g = s_dm;  // the smoothed tile reuses the depth tile's LDS (dead after the horizontal pass)
    static_assert(GH * (GW + 2) <= DH * DW, "g tile must fit in the depth tile");
    __shared__ unsigned long long s_key[4];
    __shared__ int s_any[2];
    typedef float lg_f4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) LgFinalArgs* lg_args_ptr;
    lg_args_ptr ap = (lg_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    (void)a_;

    // ---- the tile walk, in scalar registers (total < 2^31: lg_launch_final)
    // Near launch (ap->near_off): the walk runs over the batch's list of near tiles (lg_near_tiles; frame b owns the entries
    // near_off[b] .. near_off[b + 1] - 1, the tiles of its rectangle row by row) instead of over every tile of every frame.
    const int ntile = ap->tiles_x * ap->tiles_y;
    typedef const __attribute__((address_space(4))) int32_t* lg_off_ptr;
    const bool near = ap->near_off != nullptr;
    const int total = near ? ap->near_total : ntile * ap->B;
    const int xcd = (int)(blockIdx.x & 7u), tq = total >> 3, tr = total & 7;
    const int xcd_first = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
    const int xcd_count = tq + (xcd < tr ? 1 : 0);
    // tiles per workgroup (ap->tpw > 0): workgroup j of the XCD takes the tpw consecutive tiles j * tpw ...; otherwise one tile
    // each, or, as resident workgroups, tiles j, j + n, j + 2n ... of the XCD's range
    const int tpw = near ? ap->near_tpw : ap->tpw;
    const int stride = tpw > 0 ? 1 : (int)((gridDim.x + 7u) >> 3);
    int it = (int)(blockIdx.x >> 3) * (tpw > 0 ? tpw : 1);
    const int it_end = tpw > 0 ? min(it + tpw, xcd_count) : xcd_count;
    if (it >= it_end) return;
    int frame = __builtin_amdgcn_readfirstlane((xcd_first + it) / ntile);
    int tile = xcd_first + it - frame * ntile;
    const int step_f = __builtin_amdgcn_readfirstlane(stride / ntile), step_t = stride - step_f * ntile;
    int par = 0;   // s_any slot: flips at every tile that takes the bit-row test (tiles far from the leaf take no barrier)
    for (; it < it_end;
         it += stride, frame += step_f, tile += step_t, frame += (tile >= ntile ? 1 : 0), tile -= (tile >= ntile ? ntile : 0)) {
    asm volatile("" : "+s"(ap));
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int tiles_x = ap->tiles_x;
    const int H = ap->H, W = ap->W, WW = ap->WW;
    int li = 0;
    if (near) {   // the frame of list entry li: the last one that starts at or before it (scalar binary search; frames without near tiles own no entry)
        lg_off_ptr noff = (lg_off_ptr)ap->near_off;
        li = ap->near_base + xcd_first + it;   // (the batch's entry: a launch over a range of frames starts at its first frame's)
        int lo = 0, hi = ap->B;   // near_off[lo] <= li < near_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (noff[mid] <= li) lo = mid; else hi = mid;
        }
        frame = lo;
        li -= noff[lo];
    }
    // the frame's near tiles: can a tile's bit-row test below meet the mask's bounding box at all?  (win / fp / maxfix were
    // written by earlier kernels and are only read here: constant-address-space loads, i.e. the scalar cache, instead of a vector
    // load + readfirstlane per value)
    int rx0, rx1, ry0, ry1;
    {
        const __attribute__((address_space(4))) LgWin* wp = (const __attribute__((address_space(4))) LgWin*)(ap->win + frame);
        lg_near_tiles(wp->bx0, wp->bx1, wp->by0, wp->by1, H, W, HALO, &rx0, &rx1, &ry0, &ry1);
    }
    if (near) {   // entry li of the rectangle, row by row (li < 8192, at most 128 tiles per row: the float quotient as below)
        const int nx = rx1 - rx0 + 1;
        const int q = __builtin_amdgcn_readfirstlane((int)(((float)li + 0.5f) * __frcp_rn((float)nx)));
        tile = (ry0 + q) * tiles_x + rx0 + (li - q * nx);
    }
    // tile < 8192, tiles_x <= 128: the float quotient of (tile + 0.5) is at least 0.5 / 128 away from an integer, its error < 0.001
    const int by = __builtin_amdgcn_readfirstlane((int)(((float)tile + 0.5f) * __frcp_rn((float)tiles_x)));
    const int bx = tile - by * tiles_x;
    const int tx0 = bx * LG_TW, ty0 = by * LG_TH;
    const size_t fo = (size_t)frame * H * W;
    const char* depth = (const char*)(ap->depth + fo);
    const char* bits = (const char*)(ap->bits + (size_t)frame * H * WW);
    const char* stemb = (const char*)(ap->stem_bits + (size_t)frame * H * WW);
    auto bits_at = [&](const char* base, int y, int w) {   // uniform base + 32-bit lane offset (saddr addressing)
        return *reinterpret_cast<const unsigned long long*>(base + (unsigned)(y * WW + w) * 8u);
    };

    const int txi = t & 15, tyi = t >> 4;
    constexpr bool vec = VEC;         // x0 % 4 == 0 always; x0 + 3 < W when W % 4 == 0
    constexpr int RPT = LG_TH / 16;   // rows per thread (16 thread rows per tile)
    static_assert(LG_TH % 16 == 0 && RPT >= 1, "tile height must be a multiple of 16");
    // distance_map is only computed inside the frame's sweep window (LgWin, tile aligned); outside it is exactly 0 and
    // this kernel writes the plane instead of reading it
    bool in_win;
    const bool near_leaf = bx >= rx0 && bx <= rx1 && by >= ry0 && by <= ry1;   // (always, in the near launch)
    {
        const __attribute__((address_space(4))) LgWin* wp = (const __attribute__((address_space(4))) LgWin*)(ap->win + frame);
        const int wx0 = wp->wx0;
        in_win = tx0 >= wx0 && tx0 < min(W, wx0 + wp->nw * ap->win_wc) && ty0 >= wp->wy0 && ty0 < wp->wy1;
    }
    // 4 floats of one plane at pixel offset `off` of this frame (uniform plane base + 32-bit byte offset)
    auto st4 = [&](int mi, unsigned off, int x0, const float* v) {
        if (SCORE && mi != LG_MAP_TRADITIONAL && mi != LG_MAP_DISTANCE && mi != LG_MAP_FLATNESS) return;   // (mi is a literal at every call)
        float* dst = ap->maps[mi];
        if (!ALL && !SCORE && !dst) return;
        if (SCORE && mi == LG_MAP_FLATNESS && !dst) return;   // (a call without a model has no gather: nobody reads flatness, the plane is not there)
#ifdef LG_FINAL_ABLATE   // timing ablation builds only (tools/build_variants.sh): wrong results by design
        if ((LG_FINAL_ABLATE & 8) && mi != LG_MAP_TRADITIONAL) return;   // arithmetic without the plane stores
#endif
        char* p = (char*)(dst + fo) + off * 4u;
        if (vec) {
            lg_f4 pk = {v[0], v[1], v[2], v[3]};
            if (ap->nt_stores) __builtin_nontemporal_store(pk, reinterpret_cast<lg_f4*>(p));  // write-once stream (measured slower)
            else *reinterpret_cast<lg_f4*>(p) = pk;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < W) reinterpret_cast<float*>(p)[j] = v[j];
        }
    };
    auto st_valid = [&](unsigned off, int x0, uint32_t vbytes) {
        if (!ALL && !SCORE && !ap->valid) return;
        uint8_t* p = ap->valid + fo + off;
        if (vec) {
            __builtin_nontemporal_store(vbytes, reinterpret_cast<uint32_t*>(p));
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < W) p[j] = (uint8_t)((vbytes >> (8 * j)) & 1u);
        }
    };
    float zero = 0.0f;
    asm volatile("" : "+v"(zero));   // (a zero the compiler cannot keep in registers across tiles)
    // ---- tile-level fast path.  A leaf covers a few per cent of the frame: when no mask bit lies in this tile's extended
    //      region (tile + the HALO-pixel reach of the Gaussian and the 3x3 Sobel), depth * mask is 0 all over it, the smoothed
    //      plane and both gradients are 0 and flatness = exp(-5 * 0) = 1 exactly; every other plane is "* mask" = 0,
    //      traditional = w_flat * 1, nothing is valid.  Such tiles never read depth and skip the stencil phases.
    //      Wave 0 looks at the DH x 3 (row, word) pairs and posts the verdict; s_any alternates between two slots so that a
    //      wave that runs ahead into the next tested tile cannot overwrite a verdict the others have not read yet.  A tile
    //      whose test cannot meet the mask's bounding box (near_leaf) is constant without it: no bit-row load, no barrier.
    //      Sparse mode (a.sparse: the caller takes no plane back; top-k and the gather read tile_state) stores nothing of
    //      a constant tile but its key and its state byte.
    if (!ap->no_skip) {
        bool any = false;
        if (near_leaf) {
            if (t < 64) {
                unsigned long long nz = 0;
                for (int e = t; e < DH * 3; e += 64) {
                    const int er = e / 3, wq = e % 3;                 // extended row, word (left neighbour, own, right neighbour)
                    const int y = lg_reflect(ty0 - HALO + er, H), wi = bx - 1 + wq;
                    if (wi >= 0 && wi < WW) {
                        unsigned long long v = bits_at(bits, y, wi);
                        if (wq == 0) v >>= 56;                        // columns tx0-8 .. tx0-1 (halo 4 + reflection slack)
                        if (wq == 2) v &= 0xffull;                    // columns tx0+64 .. tx0+71
                        nz |= v;
                    }
                }
                const bool anyw = __ballot(nz != 0) != 0ull;
                if (t == 0) s_any[par] = anyw ? 1 : 0;
            }
            lg_lds_barrier();
            any = s_any[par] != 0;
            par ^= 1;
        }
        if (!any) {
            if (!ap->sparse) {
                const float flat1 = lg_const_flat(ap->flat_scale);
                const float tr1 = ap->w_flat * flat1;
                const float c_flat[4] = {flat1, flat1, flat1, flat1};
                const float c_trad[4] = {tr1, tr1, tr1, tr1};
                const float c_zero[4] = {zero, zero, zero, zero};
#pragma unroll
                for (int rr = 0; rr < RPT; rr++) {
                    const int y = ty0 + tyi + 16 * rr, x0 = tx0 + 4 * txi;
                    if (y < H && x0 < W) {
                        const unsigned off = (unsigned)(y * W + x0);
                        st4(LG_MAP_SDF, off, x0, c_zero); st4(LG_MAP_APPROACH, off, x0, c_zero); st4(LG_MAP_FLATNESS, off, x0, c_flat);
                        st4(LG_MAP_ISOLATION, off, x0, c_zero); st4(LG_MAP_ACCESS, off, x0, c_zero); st4(LG_MAP_STEM, off, x0, c_zero);
                        st4(LG_MAP_TRADITIONAL, off, x0, c_trad);
                        if (!in_win) st4(LG_MAP_DISTANCE, off, x0, c_zero);
                        st_valid(off, x0, 0u);
                    }
                }
            }
            if (t == 0) {   // arg-max key of a tile without valid pixels: score 0, largest flat index (top-k tie rule)
                const int ymax = min(ty0 + LG_TH, H) - 1, xmax = min(tx0 + LG_TW, W) - 1;
                ap->tilekeys[(size_t)frame * ntile + tile] =
                    ((unsigned long long)lg_orderable(0.0f) << 32) | (uint32_t)(ymax * W + xmax);
                if (ap->tile_state) ap->tile_state[(size_t)frame * ntile + tile] = 0;
            }
            continue;
        }
    }

    // ---- per-pixel operands of the full path, requested before the stencil phases so their latency overlaps them
    float din_pre[RPT][4];
    unsigned mnib_pre[RPT], snib_pre[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; rr++) {
        const int y = ty0 + tyi + 16 * rr, x0 = tx0 + 4 * txi;
        mnib_pre[rr] = snib_pre[rr] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) din_pre[rr][j] = 0.0f;
        if (y < H && x0 < W) {
            const unsigned sh = (unsigned)(x0 & 63);
            mnib_pre[rr] = (unsigned)(bits_at(bits, y, bx) >> sh) & 0xfu;
            snib_pre[rr] = (unsigned)(bits_at(stemb, y, bx) >> sh) & 0xfu;
            const char* dsrc = (const char*)(ap->maps[LG_MAP_DISTANCE] + fo) + (unsigned)(y * W + x0) * 4u;
            if (!in_win) {
            } else if (vec) {
                float4 v = *reinterpret_cast<const float4*>(dsrc);
                din_pre[rr][0] = v.x; din_pre[rr][1] = v.y; din_pre[rr][2] = v.z; din_pre[rr][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) din_pre[rr][j] = (x0 + j < W) ? reinterpret_cast<const float*>(dsrc)[j] : 0.0f;
            }
        }
    }

    // ---- stage dm = depth * mask over the extended tile (reflect padding of smooth_depth, image_processor.py:60)
    const bool fast = VEC && (tx0 >= 4) && (tx0 + LG_TW + 4 <= W);
    if (fast) {
        for (int idx = t; idx < DH * (DW / 4); idx += 256) {
            int er = idx / (DW / 4), g4 = idx % (DW / 4);
            int y = lg_reflect(ty0 - HALO + er, H);
            int x = tx0 - 4 + 4 * g4;
            float4 d = *reinterpret_cast<const float4*>(depth + (unsigned)(y * W + x) * 4u);
            unsigned long long wbits = bits_at(bits, y, x >> 6);
            unsigned nib = (unsigned)(wbits >> (x & 63)) & 0xfu;
            float4 o;
            o.x = (nib & 1u) ? d.x : 0.0f;
            o.y = (nib & 2u) ? d.y : 0.0f;
            o.z = (nib & 4u) ? d.z : 0.0f;
            o.w = (nib & 8u) ? d.w : 0.0f;
            *reinterpret_cast<float4*>(&s_dm[er * DW + 4 * g4]) = o;
        }
    } else {
        for (int idx = t; idx < DH * DW; idx += 256) {
            int er = idx / DW, ec = idx % DW;
            int y = lg_reflect(ty0 - HALO + er, H);
            int x = lg_reflect(tx0 - 4 + ec, W);
            float d = *reinterpret_cast<const float*>(depth + (unsigned)(y * W + x) * 4u);
            unsigned long long wbits = bits_at(bits, y, x >> 6);
            s_dm[idx] = ((wbits >> (x & 63)) & 1ull) ? d : 0.0f;
        }
    }
    lg_lds_barrier();
#ifdef LG_FINAL_ABLATE
    if (LG_FINAL_ABLATE & 16) {   // ablation build: the memory traffic of the dense path without its arithmetic
#pragma unroll
        for (int rr = 0; rr < RPT; rr++) {
            const int y = ty0 + tyi + 16 * rr, x0 = tx0 + 4 * txi;
            if (y < H && x0 < W) {
                const unsigned off = (unsigned)(y * W + x0);
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = din_pre[rr][j] + s_dm[(tyi + 16 * rr + HALO) * DW + 4 + 4 * txi + j] + (float)mnib_pre[rr] + (float)snib_pre[rr];
                st4(LG_MAP_SDF, off, x0, v); st4(LG_MAP_APPROACH, off, x0, v); st4(LG_MAP_FLATNESS, off, x0, v);
                st4(LG_MAP_ISOLATION, off, x0, v); st4(LG_MAP_ACCESS, off, x0, v); st4(LG_MAP_STEM, off, x0, v);
                st4(LG_MAP_TRADITIONAL, off, x0, v);
                if (!in_win) st4(LG_MAP_DISTANCE, off, x0, v);
                st_valid(off, x0, 0u);
            }
        }
        lg_lds_barrier();
        continue;
    }
#endif
    // ---- separable (2R+1)-tap Gaussian; g is stored at the *reflect-padded* coordinates the Sobel stage reads
    //      (F.pad(g,(1,1,1,1),'reflect'), grasp_point_selector.py:648): g_ext(e) = G(reflect1(e)).
    // Work split without div/mod: thread t owns column (t & 63) for rows (t >> 6) + 4k; the two extra halo
    // columns (64, 65) are covered by the first threads afterwards.
    {
        float kw[2 * R + 1];
#pragma unroll
        for (int i = 0; i < 2 * R + 1; i++) kw[i] = ap->k1[i];
        auto tap_row = [&](const float* p) { return lg_tap_row<R>(kw, p); };   // taps in ascending order, like the 5-tap form this generalises
        auto tap_col = [&](const float* p) { return lg_tap_col<R, GW>(kw, p); };
        const int ec = t & 63;
        int lc = lg_reflect(tx0 - 1 + ec, W) - (tx0 - 4);
        lc = lc < R ? R : (lc > DW - 1 - R ? DW - 1 - R : lc);
#pragma unroll
        for (int k = 0; k < (DH + 3) / 4; k++) {
            const int er = (t >> 6) + 4 * k;
            if (er < DH) s_h[er * GW + ec] = tap_row(&s_dm[er * DW + lc - R]);
        }
        if (t < 2 * DH) {
            const int er = t >> 1, ec2 = 64 + (t & 1);
            int lc2 = lg_reflect(tx0 - 1 + ec2, W) - (tx0 - 4);
            lc2 = lc2 < R ? R : (lc2 > DW - 1 - R ? DW - 1 - R : lc2);
            s_h[er * GW + ec2] = tap_row(&s_dm[er * DW + lc2 - R]);
        }
        lg_lds_barrier();
#pragma unroll
        for (int k = 0; k < (GH + 3) / 4; k++) {
            const int gr = (t >> 6) + 4 * k;
            if (gr < GH) {
                int lr = lg_reflect(ty0 - 1 + gr, H) - (ty0 - HALO);
                lr = lr < R ? R : (lr > DH - 1 - R ? DH - 1 - R : lr);
                s_g[gr * (GW + 2) + ec] = tap_col(&s_h[(lr - R) * GW + ec]);
            }
        }
        if (t < 2 * GH) {
            const int gr = t >> 1, ec2 = 64 + (t & 1);
            int lr = lg_reflect(ty0 - 1 + gr, H) - (ty0 - HALO);
            lr = lr < R ? R : (lr > DH - 1 - R ? DH - 1 - R : lr);
            s_g[gr * (GW + 2) + ec2] = tap_col(&s_h[(lr - R) * GW + ec2]);
        }
    }
    lg_lds_barrier();

    // ---- per-pixel planes
    const __attribute__((address_space(4))) LgFrameParams* fpp = (const __attribute__((address_space(4))) LgFrameParams*)(ap->fp + frame);
    const __attribute__((address_space(4))) uint32_t* mfp = (const __attribute__((address_space(4))) uint32_t*)(ap->maxfix + frame * LG_MF);
    const LgPixFrame pf = lg_pix_frame(ap, fpp, mfp);
    unsigned long long best = 0;
#pragma unroll
    for (int rr = 0; rr < RPT; rr++) {
        const int ly = tyi + 16 * rr;
        const int y = ty0 + ly;
        const int x0 = tx0 + 4 * txi;
        if (y < H && x0 < W) {
            const unsigned off = (unsigned)(y * W + x0);
            const unsigned mnib = mnib_pre[rr], snib = snib_pre[rr];
            const float* din = din_pre[rr];
            // flatness first: Sobel cross-correlation on the smoothed plane, exp(-5 |grad|) (:646-655); its 18 operands
            // are dead before the other planes' arithmetic starts
            float o_flat[4];
            {
                const float* g0 = &s_g[(ly + 0) * (GW + 2) + 4 * txi];
                const float* g1 = g0 + (GW + 2);
                const float* g2 = g1 + (GW + 2);
                float ga[6], gb[6], gc[6];
                // 16-byte + 8-byte LDS reads (row stride 272 B keeps them aligned): no bank conflicts
                const float4 a4 = *reinterpret_cast<const float4*>(g0), b4 = *reinterpret_cast<const float4*>(g1),
                             c4 = *reinterpret_cast<const float4*>(g2);
                const float2 a2 = *reinterpret_cast<const float2*>(g0 + 4), b2 = *reinterpret_cast<const float2*>(g1 + 4),
                             c2 = *reinterpret_cast<const float2*>(g2 + 4);
                ga[0] = a4.x; ga[1] = a4.y; ga[2] = a4.z; ga[3] = a4.w; ga[4] = a2.x; ga[5] = a2.y;
                gb[0] = b4.x; gb[1] = b4.y; gb[2] = b4.z; gb[3] = b4.w; gb[4] = b2.x; gb[5] = b2.y;
                gc[0] = c4.x; gc[1] = c4.y; gc[2] = c4.z; gc[3] = c4.w; gc[4] = c2.x; gc[5] = c2.y;
                lg_flat4<VEC && (ALL || SCORE)>(ga, gb, gc, ap->flat_scale, o_flat);
            }
            st4(LG_MAP_FLATNESS, off, x0, o_flat);
            if (!in_win) { const float z4[4] = {zero, zero, zero, zero}; st4(LG_MAP_DISTANCE, off, x0, z4); }
            float o_trad[4];
            uint32_t vbytes = 0;
            const float w_flat = ap->w_flat;
            // A leaf covers a few per cent of a frame: when no lane of this wave sits on the mask every plane but
            // flatness is exactly zero (they are all "* mask"), traditional = w_flat * flatness and nothing is
            // valid.  The wave-uniform branch skips the geometry / SDF / isolation arithmetic for those rows.
            const bool wave_on_mask = (ap->no_skip & 2) || __ballot(mnib != 0) != 0ull;
            if (wave_on_mask) {
                float o_sdf[4], o_app[4], o_iso[4], o_acc[4], o_stem[4];
                bool o_valid[4];
                vbytes = lg_pixels4<!SCORE>(ap, pf, y, x0, H, W, mnib, snib, din, o_flat, w_flat, o_sdf, o_app, o_iso, o_acc, o_stem,
                                            o_trad, o_valid);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x0 + j < W) {
                        unsigned long long key =
                            ((unsigned long long)lg_orderable(lg_valid_score(o_trad[j], o_valid[j])) << 32) | (uint32_t)(y * W + x0 + j);
                        best = key > best ? key : best;
                    }
                st4(LG_MAP_SDF, off, x0, o_sdf);
                st4(LG_MAP_APPROACH, off, x0, o_app);
                st4(LG_MAP_ISOLATION, off, x0, o_iso);
                st4(LG_MAP_ACCESS, off, x0, o_acc);
                st4(LG_MAP_STEM, off, x0, o_stem);
            } else {
                const float z4[4] = {zero, zero, zero, zero};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    o_trad[j] = w_flat * o_flat[j];  // (0.4*0 + 0.3*0 + 0.2*flat + 0.1*0) * (1 - 0), same float32 operations' result
                    if (x0 + j < W) {
                        unsigned long long key = ((unsigned long long)lg_orderable(0.0f) << 32) | (uint32_t)(y * W + x0 + j);
                        best = key > best ? key : best;
                    }
                }
                st4(LG_MAP_SDF, off, x0, z4);
                st4(LG_MAP_APPROACH, off, x0, z4);
                st4(LG_MAP_ISOLATION, off, x0, z4);
                st4(LG_MAP_ACCESS, off, x0, z4);
                st4(LG_MAP_STEM, off, x0, z4);
            }
            st4(LG_MAP_TRADITIONAL, off, x0, o_trad);
            st_valid(off, x0, vbytes);
        }
    }
    best = lg_wave_max_u64(best);
    if ((t & 63) == 0) s_key[t >> 6] = best;
    lg_lds_barrier();   // (also orders this tile's LDS reads before the next tile's writes)
    if (t == 0) {
        unsigned long long k = s_key[0];
        k = s_key[1] > k ? s_key[1] : k;
        k = s_key[2] > k ? s_key[2] : k;
        k = s_key[3] > k ? s_key[3] : k;
        ap->tilekeys[(size_t)frame * ntile + tile] = k;
        if (ap->tile_state) ap->tile_state[(size_t)frame * ntile + tile] = 1;
    }
    }   // tile walk
}

// Launch form of sparse mode (LgFinalArgs::sparse), where nearly every workgroup of the one-per-tile form has only a key and a
// state byte to store: consecutive tiles per workgroup, or resident workgroups per CU (0 = off; LG_FINAL_TPW / LG_FINAL_PERSIST
// override).  Benchmark headline, 256 frames of 1080p, one box: one tile per workgroup 0.70 ms; 4 / 8 / 16 / 32 / 64 / 128 tiles
// per workgroup 0.48 / 0.45 / 0.44-0.46 / 0.44-0.45 / 0.51 / 0.63 ms; resident walk with 8 / 2 workgroups per CU 0.53 / 0.96 ms.
// One tile per workgroup launches 518 k nearly empty workgroups; past 32 tiles the leaf tiles' stencil work collects on too
// few workgroups.
// The near launch (LgFinalArgs::near_off) needs neither: its grid holds the tiles around the leaves only (lg_near_tiles: 43 008
// of the headline's 522 240, 32 928 of them on the stencil path), one per workgroup, and takes 0.262 ms where the form above
// takes 0.436-0.438 (kernel trace); the other tiles' keys and state bytes come from lg_near_tiles_kernel (0.008 ms, beside the
// distance transform).  lg_select_grasp* uses it in sparse mode; the form above stays for LG_FINAL_NEAR=0, the sub-batch
// pipeline and the experiment switches.
#ifndef LG_FINAL_SPARSE_TPW
#define LG_FINAL_SPARSE_TPW 16
#endif
#ifndef LG_FINAL_SPARSE_PERSIST
#define LG_FINAL_SPARSE_PERSIST 0
#endif
void lg_launch_final(const LgFinalArgs& a_in, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    long long total = (long long)a_in.tiles_x * a_in.tiles_y * a_in.B;   // < 2^31: tiles_x * tiles_y <= 8192 (make_plan), B is an int count of frames that fit in memory
    // Launch form.  Dense mode: one workgroup per tile by default (sparse mode: LG_FINAL_SPARSE_TPW above): on real frames
    // most tiles take the constant path and the dispatcher's own load balancing beats a fixed stride (2.71 vs 3.12 ms per 256
    // frames).  LG_FINAL_PERSIST=n (a.persist): n resident
    // workgroups per CU (a multiple of 8 workgroups, so that blockIdx % 8 stays the XCD) walk the tiles.  With every tile on
    // the stencil path the walk measured 5 % faster on three boxes (2.10 vs 2.21 ms per 128 frames; its arithmetic alone 1.14
    // vs 1.42 ms) and 25 % SLOWER on a fourth, faster one (2.28-2.33 vs 1.80-1.87 ms): a wave's loads for its next tile queue
    // behind its own plane stores (vmcnt retires in order), which costs more the faster the memory side is.  Off by default.
    static const int cus = [] {
        int dev = 0, n = 256;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n;
    }();
    const int per_cu = a_in.persist >= 0 ? a_in.persist : a_in.sparse ? LG_FINAL_SPARSE_PERSIST : 0;
    const int resident = per_cu > 0 ? std::max(8, cus * per_cu / 8 * 8) : 0;
    // LG_FINAL_TPW=n (a.tpw): n consecutive tiles per workgroup (experiment: 2 / 4 / 8 change the benchmark launch by -1 / +1 / +3 %,
    // the dense launch within the noise: the workgroup launch rate is not what limits either)
    LgFinalArgs a = a_in;
    // Near launch (a.near_off; the caller offers it in sparse mode only and never beside the experiment switches above): the
    // list of near tiles takes the place of the tile grid, near_tpw consecutive entries per workgroup.  An empty list launches
    // nothing: every tile of the batch is a far tile and has its key and state byte already.
    const bool near = a.near_off != nullptr;
    if (near) {
        if (a.near_total <= 0) {
            if (ev_start && ev_stop) { hipEventRecord(ev_start, s); hipEventRecord(ev_stop, s); }
            return;
        }
        total = a.near_total;
        a.near_tpw = std::max(1, a.near_tpw);
    }
    const bool walk = !near && resident && total > 2ll * resident;
    a.tpw = walk ? 0 : std::max(0, a_in.tpw >= 0 ? a_in.tpw : a.sparse ? LG_FINAL_SPARSE_TPW : 0);
    const int tpw = near ? a.near_tpw : a.tpw;
    const long long per_xcd = (total + 7) / 8;
    const unsigned grid = (unsigned)(walk ? resident : tpw > 1 ? 8 * ((per_xcd + tpw - 1) / tpw) : total);
    if (a.tpw == 1) a.tpw = 0;
    if (a.near_tpw == 1) a.near_tpw = 0;
    bool all = a.valid != nullptr;
    for (int i = 0; i < LG_NUM_MAPS; i++) all = all && a.maps[i] != nullptr;
    const bool vec = (a.W & 3) == 0;
    const bool score = a.score_only != 0;   // (the caller sets it in sparse mode only: traditional, distance and validity are there)
    void (*k)(LgFinalArgs) = nullptr;
#define LG_FINAL_PICK(RR)                                                                                  \
    k = vec ? (score ? lg_final_kernel<true, false, RR, true> : all ? lg_final_kernel<true, true, RR> : lg_final_kernel<true, false, RR>)    \
            : (score ? lg_final_kernel<false, false, RR, true> : all ? lg_final_kernel<false, true, RR> : lg_final_kernel<false, false, RR>)
    switch (a.gauss_r) {   // make_plan admits gaussian_size 1, 3, 5, 7 only
        case 0: LG_FINAL_PICK(0); break;
        case 1: LG_FINAL_PICK(1); break;
        case 3: LG_FINAL_PICK(3); break;
        default: LG_FINAL_PICK(2); break;
    }
#undef LG_FINAL_PICK
    if (ev_start && ev_stop)  // events stamped by the command processor right around this dispatch
        hipExtLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, ev_start, ev_stop, 0, a);
    else
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, a);
}

// ============================================================================ near tiles of a batch
// In front of the near launch of lg_final_kernel, beside the distance transform.  One thread per (frame, tile): a tile outside
// its frame's rectangle (lg_near_tiles) gets the constant path's key -- score 0, largest flat index of the tile -- and state
// byte 0.  Workgroup 0 then scans the frames' near counts into near_off (thread = frame, frames t, t + 256, ... in rounds with
// a running base, as lg_survivors_kernel).  No atomics: the same output on every run.
__global__ __launch_bounds__(256) void lg_near_tiles_kernel(const LgWin* __restrict__ win, int B, int H, int W, int halo,
                                                            int32_t* __restrict__ near_off, int32_t* __restrict__ near_off_h,
                                                            unsigned long long* __restrict__ tilekeys,
                                                            uint8_t* __restrict__ tile_state) {
    const int tiles_x = (W + LG_TW - 1) / LG_TW, tiles_y = (H + LG_TH - 1) / LG_TH, ntile = tiles_x * tiles_y;
    const int t = threadIdx.x;
    int x0, x1, y0, y1;
    const long long i = (long long)blockIdx.x * 256 + t;   // < 2^31 (lg_launch_final)
    if (i < (long long)B * ntile) {
        const int frame = (int)(i / ntile), tile = (int)(i - (long long)frame * ntile);
        const int by = tile / tiles_x, bx = tile - by * tiles_x;
        lg_near_tiles(win[frame], H, W, halo, &x0, &x1, &y0, &y1);
        if (!(bx >= x0 && bx <= x1 && by >= y0 && by <= y1)) {
            const int ymax = min(by * LG_TH + LG_TH, H) - 1, xmax = min(bx * LG_TW + LG_TW, W) - 1;
            tilekeys[i] = ((unsigned long long)lg_orderable(0.0f) << 32) | (uint32_t)(ymax * W + xmax);
            tile_state[i] = 0;
        }
    }
    if (blockIdx.x != 0) return;
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + t;
        const int c = b < B ? lg_near_tiles(win[b], H, W, halo, &x0, &x1, &y0, &y1) : 0;
        int incl = c;   // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int pos = s_base + incl - c;
        for (int w = 0; w < wave; w++) pos += s_wave[w];
        __syncthreads();   // everyone has read s_base and s_wave
        if (t == 255) s_base = pos + c;
        if (b < B) {
            near_off[b] = pos;
            if (near_off_h) near_off_h[b] = pos;   // (the host's pinned copy through its device alias)
        }
        __syncthreads();
    }
    if (t == 0) {
        near_off[B] = s_base;
        if (near_off_h) near_off_h[B] = s_base;
    }
}

void lg_launch_near_tiles(const LgWin* win, int B, int H, int W, int halo, int32_t* near_off, int32_t* near_off_host_dev,
                          unsigned long long* tilekeys, uint8_t* tile_state, hipStream_t s) {
    const long long total = (long long)((W + LG_TW - 1) / LG_TW) * ((H + LG_TH - 1) / LG_TH) * B;
    hipLaunchKernelGGL(lg_near_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, win, B, H, W, halo, near_off,
                       near_off_host_dev, tilekeys, tile_state);
}

// ============================================================================ ImageProcessor.smooth_depth on its own
// image_processor.py:56-64: F.pad(depth, size // 2 on every side, 'reflect') then F.conv2d with the size x size Gaussian (a
// cross-correlation; the kernel is symmetric).  Output (H + 2P - S + 1) x (W + 2P - S + 1), P = S / 2: the input's shape for odd
// S, one row and one column more for even S (what torch returns there).  Separable: rows, then columns, taps in ascending
// order -- the same two passes as the stencil phase of lg_final_kernel.  Tile 64 x 16 outputs, 256 threads, any 1 <= S <= 15.
__global__ __launch_bounds__(256) void lg_smooth_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                        int Ho, int Wo, int S, LgGaussTaps taps) {
    constexpr int TW = 64, TH = 16, MAXS = LG_MAX_GAUSS;
    __shared__ float s_in[(TH + MAXS - 1) * (TW + MAXS - 1)];
    __shared__ float s_row[(TH + MAXS - 1) * TW];
    const int t = threadIdx.x, P = S >> 1;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const float* in = src + (size_t)blockIdx.z * H * W;
    float* out = dst + (size_t)blockIdx.z * Ho * Wo;
    const int IW = TW + S - 1, IH = TH + S - 1;
    for (int i = t; i < IH * IW; i += 256) {
        const int er = i / IW, ec = i - er * IW;
        // output (y, x) reads padded[y + i][x + j] = in[reflect(y + i - P)][reflect(x + j - P)]; rows / columns past the output
        // (partial tiles) are clamped by lg_reflect and never stored
        s_in[i] = in[(size_t)lg_reflect(ty0 + er - P, H) * W + lg_reflect(tx0 + ec - P, W)];
    }
    __syncthreads();
    for (int i = t; i < IH * TW; i += 256) {
        const int er = i >> 6, c = i & 63;
        const float* p = &s_in[er * IW + c];
        float acc = taps.k[0] * p[0];
        for (int j = 1; j < S; j++) acc += taps.k[j] * p[j];
        s_row[i] = acc;
    }
    __syncthreads();
    for (int i = t; i < TH * TW; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int y = ty0 + r, x = tx0 + c;
        if (y < Ho && x < Wo) {
            const float* p = &s_row[r * TW + c];
            float acc = taps.k[0] * p[0];
            for (int j = 1; j < S; j++) acc += taps.k[j] * p[j * TW];
            out[(size_t)y * Wo + x] = acc;
        }
    }
}

void lg_launch_smooth(const float* src, float* dst, int B, int H, int W, int S, const LgGaussTaps& taps, hipStream_t s) {
    const int P = S / 2, Ho = H + 2 * P - S + 1, Wo = W + 2 * P - S + 1;
    hipLaunchKernelGGL(lg_smooth_kernel, dim3((Wo + 63) / 64, (Ho + 15) / 16, B), dim3(256), 0, s, src, dst, H, W, Ho, Wo, S, taps);
}
