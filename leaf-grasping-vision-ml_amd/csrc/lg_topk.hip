// Tile keys, the greedy spaced top-k over them, and the list of candidates that go through the CNN.
// Reference semantics: scripts/utils/grasp_point_selector.py (cited per kernel); design: DESIGN.md.
#include "lg_topk.h"
#include "lg_pixel.h"
#include "lg_wave.h"

#include <stdlib.h>

__global__ __launch_bounds__(256) void lg_tilekeys_kernel(const float* __restrict__ trad,
                                                          const uint8_t* __restrict__ valid,
                                                          unsigned long long* __restrict__ tilekeys, int H, int W,
                                                          int tiles_x, int tiles_y) {
    __shared__ unsigned long long s_key[4];
    const int ntile = tiles_x * tiles_y;
    const int frame = blockIdx.y, tile = blockIdx.x;
    const int bx = tile % tiles_x, by = tile / tiles_x;
    const size_t fo = (size_t)frame * H * W;
    unsigned long long best = 0;
    for (int i = threadIdx.x; i < LG_TW * LG_TH; i += 256) {
        int x = bx * LG_TW + (i % LG_TW), y = by * LG_TH + (i / LG_TW);
        if (x < W && y < H) {
            size_t o = fo + (size_t)y * W + x;
            float sc = lg_valid_score(trad[o], valid[o] != 0);
            unsigned long long key = ((unsigned long long)lg_orderable(sc) << 32) | (uint32_t)(y * W + x);
            best = key > best ? key : best;
        }
    }
    best = lg_wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long k = s_key[0];
        for (int w = 1; w < 4; w++) k = s_key[w] > k ? s_key[w] : k;
        tilekeys[(size_t)frame * ntile + tile] = k;
    }
}

// ============================================================================ greedy spaced top-k
// GraspPointSelector._get_candidate_points (grasp_point_selector.py:447-482) without the full sort:
// repeat k times { argmax over not-yet-suppressed pixels (score desc, flat index desc);
//                  suppress every pixel within Chebyshev distance 2*min_dist of the pick }.
// Equivalent to the reference's greedy walk over the descending argsort (a pixel is accepted iff its
// (2d+1)^2 window meets no earlier window, i.e. iff it is > 2d away from every accepted point).
// One LG_TOPK_T-thread workgroup per frame; per-tile maxima live in LDS and only the tiles touched by a new suppression
// window (<= 8 of 64x16 pixels for the reference's 41x41 window; any number for larger min_distance) are recomputed.
// tile_state (sparse planes): a tile with state 0 has no trad / valid written; its pixels are read as the constant tile's
// (trad = w_flat * lg_const_flat(flat_scale), valid = 0) -- the same keys, tie rule included, as the written planes give.
//
// A round of the usual case (window on <= 8 tiles, W % 4 == 0) is two barriers around one round trip to L2:
//   arg-max of the tile keys -> s_best[r & 1] | barrier 1 | pick; one WAVE per touched tile recomputes its key -> s_keys | barrier 2
// The picks so far live in registers (lane q of every wave holds pick q), so the round reads no pick from LDS; s_cx / s_cy
// are written for the general form and the tail only.
#ifndef LG_TOPK_T
#define LG_TOPK_T 512   // 8 waves = one per tile of a 41 x 41 window (measured against 256 and 1024: profiles/NOTES_topk_chain.md)
#endif
#define LG_MAX_TILES 8192
#define LG_MAX_K 64
__global__ __launch_bounds__(LG_TOPK_T) void lg_topk_kernel(const float* __restrict__ trad,
                                                            const uint8_t* __restrict__ valid,
                                                            const float* __restrict__ depth,
                                                            const unsigned long long* __restrict__ tilekeys,
                                                            const uint8_t* __restrict__ tile_state, float flat_scale,
                                                            float w_flat, int H,
                                                            int W, int tiles_x, int tiles_y, int k, int md,
                                                            int32_t* __restrict__ out_xy, int32_t* __restrict__ out_n,
                                                            float* __restrict__ out_info,
                                                            unsigned long long* __restrict__ keep, int mask_is_bool) {
    static_assert(LG_TOPK_T % 64 == 0 && LG_TOPK_T >= 64 && (LG_TW * LG_TH) % LG_TOPK_T == 0, "whole waves; whole chunks per tile");
    static_assert(LG_TW == 64 && LG_TH == 16, "fast path: a wave takes a tile as 16 rows x 4 lanes x 16 pixels");
    constexpr int NW = LG_TOPK_T / 64;
    __shared__ unsigned long long s_keys[LG_MAX_TILES];
    __shared__ uint8_t s_state[LG_MAX_TILES];   // 1: the tile's planes were written (every tile when tile_state is null)
    __shared__ unsigned long long s_best[2];    // the round's arg-max, by round parity
    __shared__ int s_cx[LG_MAX_K], s_cy[LG_MAX_K];
    const int frame = blockIdx.x;
    const int ntile = tiles_x * tiles_y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t fo = (size_t)frame * H * W;
    const int sup = 2 * md;
    const float inv_w = __frcp_rn((float)W);
    for (int i = t; i < ntile; i += LG_TOPK_T) {
        s_keys[i] = tilekeys[(size_t)frame * ntile + i];
        s_state[i] = tile_state ? tile_state[(size_t)frame * ntile + i] : 1;
    }
    const float trad1 = w_flat * lg_const_flat(flat_scale);   // traditional score of a constant tile
    if (t < 2) s_best[t] = 0;
    __syncthreads();
    int n = 0;
    int pcx = 0, pcy = 0;   // lane q of every wave: pick q (q <= the current round; k <= 64)
    for (int r = 0; r < k; r++) {
        const int par = r & 1;
        unsigned long long b = 0;
        for (int i = t; i < ntile; i += LG_TOPK_T) b = s_keys[i] > b ? s_keys[i] : b;
        b = lg_wave_max_u64(b);
        if (lane == 0 && b) atomicMax(&s_best[par], b);
        __syncthreads();   // barrier 1: s_best[par] complete; every read of s_keys of this round is done
        const unsigned long long bk = s_best[par];
        if (bk == 0) break;  // every pixel is suppressed
        const int idx = (int)(uint32_t)(bk & 0xffffffffull);
        // idx < 2^24 (at most 8192 tiles of 1024 pixels): the float quotient is within 1 of idx / W
        int py = (int)(((float)idx + 0.5f) * inv_w);
        py -= (py * W > idx) ? 1 : 0;
        py += ((py + 1) * W <= idx) ? 1 : 0;
        const int px = idx - py * W;
        if (t == 0) {
            s_cx[r] = px; s_cy[r] = py;
            out_xy[((size_t)frame * k + r) * 2 + 0] = px;
            out_xy[((size_t)frame * k + r) * 2 + 1] = py;
            // No barrier between the read of s_best above and its reset: the round's arg-max alternates between two words.
            // s_best[par ^ 1] was last read behind barrier 1 of round r - 1, and every thread has since passed barrier 1 of this
            // round; it is next written (atomicMax of round r + 1) behind the barrier that ends this round, which this thread
            // reaches after the store.  s_best[par] itself is not written again before round r + 2's reset in round r + 1.
            s_best[par ^ 1] = 0;
        }
        if (lane == r) { pcx = px; pcy = py; }
        n = r + 1;
        // tiles touched by the new suppression window
        const int tx_lo = max(px - sup, 0) / LG_TW, tx_hi = min(px + sup, W - 1) / LG_TW;
        const int ty_lo = max(py - sup, 0) / LG_TH, ty_hi = min(py + sup, H - 1) / LG_TH;
        const int ntx = tx_hi - tx_lo + 1, nty = ty_hi - ty_lo + 1;
        const int naff = ntx * nty;
        if (naff <= 8 && (W & 3) == 0) {
            // The usual case (min_distance 10: a 41 x 41 window touches at most 2 x 4 tiles), kept short: the whole kernel runs on
            // ONE CU per frame and every round is a dependent chain, so what counts is the instructions each SIMD issues per round.
            // One wave per touched tile; lane: row lane >> 2 of the tile, 16 consecutive pixels: four 16-byte score loads + four
            // 4-byte validity loads, all issued before anything is looked at.  The wave owns the tile's key: a plain store of the
            // wave's arg-max replaces clear + barrier + atomicMax -- nobody else writes s_keys[tile] in this round, the reads of
            // this round's arg-max lie in front of barrier 1, those of the next round behind barrier 2.
            for (int ta = wave; ta < naff; ta += NW) {       // (wave-uniform)
                int ry = 0, rx = ta;
                while (rx >= ntx) { rx -= ntx; ry++; }       // (ntx <= 8: a few wave-uniform iterations instead of a division)
                const int tile = (ty_lo + ry) * tiles_x + tx_lo + rx;
                const int tx0 = (tx_lo + rx) * LG_TW, ty0 = (ty_lo + ry) * LG_TH;
                const int y = ty0 + (lane >> 2), x0 = tx0 + (lane & 3) * 16;
                const bool in = y < H && x0 < W;
                const size_t o = in ? fo + (size_t)y * W + x0 : fo;
                // W % 4 == 0: groups of four pixels are inside or outside as a whole; a group outside loads pixel 0 of the frame
                uint32_t inm = 0;
#pragma unroll
                for (int g = 0; g < 4; g++) inm |= (in && x0 + 4 * g < W) ? 0xFu << (4 * g) : 0u;
                float4 s4[4];
                uint32_t v4[4];
                if (s_state[tile] != 0) {                    // (uniform over the wave)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const size_t og = (inm >> (4 * g)) & 1u ? o + 4 * g : fo;
                        s4[g] = *reinterpret_cast<const float4*>(trad + og);
                        v4[g] = *reinterpret_cast<const uint32_t*>(valid + og);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; g++) { s4[g] = make_float4(trad1, trad1, trad1, trad1); v4[g] = 0u; }
                }
                // earlier picks (this round's included) whose window reaches this tile: one ballot over the lanes that hold them;
                // each leaves one interval of this lane's 16 pixels dead
                const unsigned long long rel = __ballot(lane <= r && pcx + sup >= tx0 && pcx - sup <= tx0 + LG_TW - 1 &&
                                                        pcy + sup >= ty0 && pcy - sup <= ty0 + LG_TH - 1);
                uint32_t dead = 0;
                for (unsigned long long m = rel; m; m &= m - 1) {
                    const int q = __builtin_ctzll(m);
                    const int cxq = __builtin_amdgcn_readlane(pcx, q), cyq = __builtin_amdgcn_readlane(pcy, q);
                    const int lo = max(cxq - sup - x0, 0), hi = min(cxq + sup - x0, 15);
                    dead |= (lo <= hi && abs(y - cyq) <= sup) ? (2u << hi) - (1u << lo) : 0u;
                }
                const uint32_t alive = inm & ~dead;
                const float sc[16] = {s4[0].x, s4[0].y, s4[0].z, s4[0].w, s4[1].x, s4[1].y, s4[1].z, s4[1].w,
                                      s4[2].x, s4[2].y, s4[2].z, s4[2].w, s4[3].x, s4[3].y, s4[3].z, s4[3].w};
                // the lane's arg-max: orderable(anything alive) >= 0x007fffff > 0, zero = suppressed / outside the image; the flat
                // index grows with j, so `>=` gives a tie to the higher index
                uint32_t bs = 0, bj = 0;
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t vb = (v4[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    const uint32_t v = (alive >> j) & 1u ? lg_orderable(lg_valid_score(sc[j], vb != 0)) : 0u;
                    if (v >= bs) { bs = v; bj = j; }
                }
                // ... and the wave's: the flat index grows with the lane too (row-major, four lanes per row)
                const unsigned long long best = lg_wave_argmax_lane_ordered(bs, (uint32_t)(y * W + x0) + bj);
                if (lane == 0) s_keys[tile] = best;
            }
            __syncthreads();   // barrier 2: the touched tiles' keys are in place for the next round's arg-max
            continue;
        }
        __syncthreads();  // s_cx/s_cy visible
        for (int i = t; i < naff; i += LG_TOPK_T)   // any window size: a large min_distance touches more tiles than there are threads
            s_keys[(ty_lo + i / ntx) * tiles_x + tx_lo + i % ntx] = 0;
        __syncthreads();
        // earlier picks whose suppression window reaches the affected tiles at all (usually the new pick and a neighbour or
        // two): the per-pixel test below walks these, not all r + 1 picks
        unsigned long long rel = 0;
        {
            const int xlo = tx_lo * LG_TW, xhi = tx_hi * LG_TW + LG_TW - 1, ylo = ty_lo * LG_TH, yhi = ty_hi * LG_TH + LG_TH - 1;
            for (int q = 0; q <= r; q++)
                if (s_cx[q] + sup >= xlo && s_cx[q] - sup <= xhi && s_cy[q] + sup >= ylo && s_cy[q] - sup <= yhi) rel |= 1ull << q;
        }
        // General form (any window size, any width): chunks of LG_TOPK_T pixels of a tile; the loads of up to 12 chunks are issued
        // together (one round trip to L2 / HBM instead of one per chunk).
        constexpr int CPT = LG_TW * LG_TH / LG_TOPK_T;
        const int chunks = naff * CPT;
        constexpr int GRP = 12;
        for (int cb = 0; cb < chunks; cb += GRP) {
            float sc_[GRP];
            int idx_[GRP], tile_[GRP], x_[GRP], y_[GRP];
            unsigned off_[GRP];
            // addresses first, then every load of the group back to back with nothing conditional on a loaded value in between
            // (written as `valid[o] ? trad[o] : 0` per chunk, hipcc issued byte load -> wait -> branch -> float load -> wait for
            // each chunk)
#pragma unroll
            for (int g = 0; g < GRP; g++) {
                const int c = min(cb + g, chunks - 1);
                const int ta = c / CPT;
                const int tile = (ty_lo + ta / ntx) * tiles_x + tx_lo + ta % ntx;
                const int li = (c % CPT) * LG_TOPK_T + t;
                const int x = (tile % tiles_x) * LG_TW + (li % LG_TW), y = (tile / tiles_x) * LG_TH + (li / LG_TW);
                const bool inb = x < W && y < H;
                tile_[g] = tile; x_[g] = x; y_[g] = y;
                idx_[g] = inb ? y * W + x : -1;
                off_[g] = inb ? (unsigned)(y * W + x) : 0u;   // (outside the image: pixel 0 of the frame, loaded and ignored)
            }
            uint8_t vv_[GRP];
            float tt_[GRP];
#pragma unroll
            for (int g = 0; g < GRP; g++) {
                const bool mat = s_state[tile_[g]] != 0;
                vv_[g] = mat ? __builtin_nontemporal_load(valid + fo + off_[g]) : (uint8_t)0;
                tt_[g] = mat ? __builtin_nontemporal_load(trad + fo + off_[g]) : trad1;
            }
#pragma unroll
            for (int g = 0; g < GRP; g++) sc_[g] = idx_[g] >= 0 ? lg_valid_score(tt_[g], vv_[g] != 0) : 0.0f;
#pragma unroll
            for (int g = 0; g < GRP; g++) {
                if (cb + g < chunks) {   // uniform across the workgroup
                    uint32_t score = 0;   // orderable(anything alive) >= 0x00800000 > 0: zero = suppressed / outside the image
                    if (idx_[g] >= 0) {
                        const int x = x_[g], y = y_[g];
                        bool dead = false;
                        for (unsigned long long m = rel; m; m &= m - 1) {
                            const int q = __builtin_ctzll(m);
                            dead |= (abs(x - s_cx[q]) <= sup) && (abs(y - s_cy[q]) <= sup);
                        }
                        if (!dead) score = lg_orderable(sc_[g]);
                    }
                    // within a wave of a chunk the flat index grows with the lane (li = chunk * LG_TOPK_T + t, one tile row per wave): the cheaper lane-ordered arg-max
                    const unsigned long long key = lg_wave_argmax_lane_ordered(score, (uint32_t)idx_[g]);
                    if ((t & 63) == 0 && key) atomicMax(&s_keys[tile_[g]], key);
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) out_n[frame] = n;
    // traditional score + depth at the picks, gathered once after the walk (a dependent global load inside
    // every round would sit on the critical path of the next arg-max)
    float tr = 0.0f;
    if (out_info && t < n) {
        const size_t o = fo + (size_t)s_cy[t] * W + s_cx[t];
        const int tile = (s_cy[t] / LG_TH) * tiles_x + s_cx[t] / LG_TW;
        tr = s_state[tile] ? trad[o] : trad1;
        out_info[((size_t)frame * k + t) * 2 + 0] = tr;
        out_info[((size_t)frame * k + t) * 2 + 1] = depth ? depth[o] : 0.0f;
    }
    // which candidates the CNN rescoring can still take (lg_finish_kernel's eligibility and lg_cnn_cannot_win against
    // candidate 0, on the float32 scores written above): the first wave holds all n <= 64 of them
    if (keep && out_info && t < 64) {
        const float tr0 = __shfl(tr, 0, 64);
        bool kp = false;
        if (t < n && n > 1) {
            const int x = s_cx[t], y = s_cy[t];
            const bool border = mask_is_bool && (x < 16 || y < 16 || x + 16 > W || y + 16 > H);
            kp = !border && !lg_cnn_cannot_win((double)tr, (double)tr0);
        }
        const unsigned long long m = __ballot(kp);
        if (t == 0) keep[frame] = m;
    }
}

// ============================================================================ survivor list
// keep[b] (lg_topk_kernel) -> the compact list of (frame, candidate) pairs that go through the CNN, in (frame, candidate)
// order, its length and the map back.  One 1024-thread workgroup, thread = frame (frames t, t + 1024, ... in rounds with a
// running base): popcount, exclusive scan over the workgroup, then every thread writes its frame's K map entries and its list
// entries.  No atomics: the order does not depend on timing.
__global__ __launch_bounds__(1024) void lg_survivors_kernel(const unsigned long long* __restrict__ keep, int B, int K,
                                                            int32_t* __restrict__ list, int32_t* __restrict__ slot,
                                                            int32_t* __restrict__ count) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int b = b0 + t;
        const unsigned long long m = b < B ? keep[b] : 0ull;
        const int c = __popcll(m);
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
        if (t == 1023) s_base = pos + c;
        if (b < B) {
            for (int i = 0; i < K; i++) {
                const bool on = (m >> i) & 1ull;
                slot[(size_t)b * K + i] = on ? pos : -1;
                if (on) list[pos++] = b * K + i;
            }
        }
        __syncthreads();
    }
    if (t == 0) *count = s_base;
}

void lg_launch_survivors(const unsigned long long* keep, int B, int K, int32_t* list, int32_t* slot, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(lg_survivors_kernel, dim3(1), dim3(1024), 0, s, keep, B, K, list, slot, count);
}

void lg_launch_topk(const float* trad, const uint8_t* valid, const float* depth, unsigned long long* tilekeys,
                    const uint8_t* tile_state, float flat_scale, float w_flat,
                    bool keys_ready, int B, int H, int W, int k, int min_dist, int32_t* out_xy, int32_t* out_n,
                    float* out_info, hipStream_t s, unsigned long long* keep, int mask_is_bool) {
    int tiles_x = (W + LG_TW - 1) / LG_TW, tiles_y = (H + LG_TH - 1) / LG_TH;
    if (!keys_ready)   // (keys from the planes themselves: every plane written)
        hipLaunchKernelGGL(lg_tilekeys_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, s, trad, valid, tilekeys, H, W,
                           tiles_x, tiles_y);
    hipLaunchKernelGGL(lg_topk_kernel, dim3(B), dim3(LG_TOPK_T), 0, s, trad, valid, depth, tilekeys,
                       keys_ready ? tile_state : nullptr, flat_scale, w_flat, H, W, tiles_x, tiles_y, k, min_dist, out_xy,
                       out_n, out_info, keep, mask_is_bool);
}
