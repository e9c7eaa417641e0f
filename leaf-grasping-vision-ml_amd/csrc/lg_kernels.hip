// gfx950 kernels of the per-pixel grasp-scoring path (score planes, fusion, top-k, patch gather).
// Reference semantics: scripts/utils/grasp_point_selector.py (cited per kernel); design: DESIGN.md.
#include "lg_internal.h"
#include "lg_wave.h"

#include <hip/hip_ext.h>

#include <limits.h>
#include <algorithm>
#include <type_traits>
#include <stdlib.h>

// ============================================================================ helpers
// max of a 64-bit key over the wave, returned in every lane.  DPP row shifts / row broadcasts on the two
// halves (a ds_bpermute shuffle costs ~100+ cycles of latency per step; the top-k walk does 13 of these per round).
#define LG_MAX64_STEP(CTRL, RMASK)                                                            \
    {                                                                                         \
        const uint32_t oh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, RMASK, 0xf, false); \
        const uint32_t ol = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, RMASK, 0xf, false); \
        const bool take = (oh > hi) || (oh == hi && ol > lo);                                 \
        hi = take ? oh : hi;                                                                  \
        lo = take ? ol : lo;                                                                  \
    }
__device__ __forceinline__ unsigned long long lg_wave_max_u64(unsigned long long v) {
    uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    LG_MAX64_STEP(0x111, 0xf)  // row_shr:1
    LG_MAX64_STEP(0x112, 0xf)  // row_shr:2
    LG_MAX64_STEP(0x114, 0xf)  // row_shr:4
    LG_MAX64_STEP(0x118, 0xf)  // row_shr:8
    LG_MAX64_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1,3
    LG_MAX64_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2,3
    hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
    lo = (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
    return ((unsigned long long)hi << 32) | lo;
}
// (score, index) arg-max over the wave where the index grows with the lane: max of the 32-bit scores by DPP (12 instructions),
// then the highest lane holding it -- a third of the instructions of the 64-bit key reduction above, same result as
// max over (score << 32 | index).  Returns the key in every lane; all-zero scores give 0.
__device__ __forceinline__ unsigned long long lg_wave_argmax_lane_ordered(uint32_t score, uint32_t index) {
    uint32_t m = score;
#define LG_MAX32_STEP(CTRL, RMASK) { const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, CTRL, RMASK, 0xf, false); m = o > m ? o : m; }
    LG_MAX32_STEP(0x111, 0xf)  // row_shr:1
    LG_MAX32_STEP(0x112, 0xf)  // row_shr:2
    LG_MAX32_STEP(0x114, 0xf)  // row_shr:4
    LG_MAX32_STEP(0x118, 0xf)  // row_shr:8
    LG_MAX32_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1,3
    LG_MAX32_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2,3
#undef LG_MAX32_STEP
    m = (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
    if (m == 0) return 0ull;
    const unsigned long long who = __ballot(score == m);
    const int lane = 63 - __builtin_clzll(who);
    const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)index, lane);
    return ((unsigned long long)m << 32) | idx;
}
__device__ __forceinline__ uint32_t lg_orderable(float s) {  // monotone float -> uint32 map
    if (s == 0.0f) s = 0.0f;  // -0.0 -> +0.0 (numpy sorts them as equal)
    if (s != s) return 0xFFFFFFFFu;   // NaN of either sign: np.argsort puts NaN last, the reference's [::-1] puts it FIRST (:454)
    uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// valid_scores = traditional_score * valid_regions (grasp_point_selector.py:451) -- a product, not a selection: a NaN or
// infinite score (non-finite depth on the leaf) stays NaN where the pixel is not valid, and NaN leads the candidate order
__device__ __forceinline__ float lg_valid_score(float trad, bool valid) { return trad * (valid ? 1.0f : 0.0f); }
// flatness of a tile off the leaf: exp(-flat_scale * |grad 0|), evaluated at run time (lg_final_kernel's constant path; top-k and
// the gather substitute it for tiles that path left unwritten, and must get the same float, whatever flat_scale is).  Its
// traditional score is w_flat * this, one multiplication.
__device__ __forceinline__ float lg_const_flat(float flat_scale) {
    float zero = 0.0f;
    asm volatile("" : "+v"(zero));
    return __expf(-flat_scale * __builtin_amdgcn_sqrtf(zero));
}
__device__ __forceinline__ int lg_reflect(int v, int n) {  // torch 'reflect' index, clamped for safety
    if (v < 0) v = -v;
    if (v >= n) v = 2 * (n - 1) - v;
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

// ============================================================================ mask -> bit rows
// The pass also reduces every frame to its bounding box and area (LG_MF in lg_internal.h), from the words it holds in registers
// anyway: grid (blocks per frame, B), so a workgroup stays inside one frame; a thread folds the set bits it packed into four
// maxima and a count (nothing to do where it saw none -- a leaf covers a few per cent of a frame), lg_box_flush reduces them
// over the workgroup and issues at most five integer atomics, from workgroups that saw a set bit only.
struct LgBoxAcc {
    uint32_t ex0 = 0, x1 = 0, ey0 = 0, y1 = 0, cnt = 0;   // max W - 1 - x, max x, max H - 1 - y, max y, set bits
    // set bits `v` (< 2^nbits) of row y, bit j = pixel xb + j
    __device__ __forceinline__ void add(unsigned long long v, int xb, int y, int H, int W) {
        if (__ballot(v != 0) == 0) return;   // (most waves: nothing of this costs them more than the ballot)
        if (v) {
            ex0 = max(ex0, (uint32_t)(W - 1 - (xb + __builtin_ctzll(v))));
            x1 = max(x1, (uint32_t)(xb + 63 - __builtin_clzll(v)));
            ey0 = max(ey0, (uint32_t)(H - 1 - y));
            y1 = max(y1, (uint32_t)y);
            cnt += __popcll(v);
        }
    }
};
// every thread of the 256-thread workgroup calls this once, outside divergent code; s_box: 5 words of LDS
__device__ __forceinline__ void lg_box_flush(const LgBoxAcc& a, uint32_t* s_box, uint32_t* __restrict__ mf_frame) {
    const int t = threadIdx.x;
    if (t < 5) s_box[t] = 0;
    __syncthreads();
    if (__ballot(a.cnt != 0)) {   // (wave-uniform)
        const uint32_t ex0 = lg_wave_max_u32(a.ex0), x1 = lg_wave_max_u32(a.x1), ey0 = lg_wave_max_u32(a.ey0), y1 = lg_wave_max_u32(a.y1);
        uint32_t c = a.cnt;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((t & 63) == 0) {
            atomicMax(&s_box[0], ex0); atomicMax(&s_box[1], x1); atomicMax(&s_box[2], ey0); atomicMax(&s_box[3], y1);
            atomicAdd(&s_box[4], c);
        }
    }
    __syncthreads();
    if (t < 5 && s_box[4] != 0) {
        if (t < 4) atomicMax(&mf_frame[LG_BOX_X0 + t], s_box[t]);
        else atomicAdd(&mf_frame[LG_BOX_AREA], s_box[4]);
    }
}

// bits[b][y][w] bit j = mask[b][y][64w + j] != 0.  One wave-ballot per 64 pixels.
__global__ __launch_bounds__(256) void lg_pack_bits_kernel(const uint8_t* __restrict__ mask,
                                                           unsigned long long* __restrict__ bits, int H, int W, int WW,
                                                           uint32_t* __restrict__ mf) {
    __shared__ uint32_t s_box[5];
    const int lane = threadIdx.x & 63, frame = blockIdx.y;
    const int nwords = H * WW;                                   // of one frame
    const uint8_t* fm = mask + (size_t)frame * H * W;
    unsigned long long* fb = bits + (size_t)frame * nwords;
    LgBoxAcc acc;
    const int stride = (gridDim.x * 256) >> 6;
    for (int wid = (blockIdx.x * 256 + threadIdx.x) >> 6; wid < nwords; wid += stride) {   // one 64-bit word per wave
        const int row = wid / WW, w = wid - row * WW;
        const int x = w * 64 + lane;
        uint8_t m = (x < W) ? fm[(size_t)row * W + x] : (uint8_t)0;
        unsigned long long b = __ballot(m != 0);
        if (lane == 0) { fb[wid] = b; if (mf) acc.add(b, w * 64, row, H, W); }
    }
    if (mf) lg_box_flush(acc, s_box, mf + (size_t)frame * LG_MF);
}

// Vector variant (W % 16 == 0): each lane loads 16 mask bytes (1 KiB per wave instruction), four adjacent
// lanes assemble one 64-bit word.  Slot s of a row covers pixels [16s, 16s+16); slots beyond W are empty.
__global__ __launch_bounds__(256) void lg_pack_bits16_kernel(const uint8_t* __restrict__ mask,
                                                             unsigned long long* __restrict__ bits, int H, int W, int WW,
                                                             uint32_t* __restrict__ mf) {
    __shared__ uint32_t s_box[5];
    const int slots_per_row = 4 * WW, frame = blockIdx.y;
    const int nslots = H * slots_per_row;                        // of one frame; a multiple of 4
    const uint8_t* fm = mask + (size_t)frame * H * W;
    unsigned long long* fb = bits + (size_t)frame * H * WW;
    LgBoxAcc acc;
    const int stride = gridDim.x * 256;  // multiple of 4: a word's four slots stay in adjacent lanes
    for (int sid = blockIdx.x * 256 + threadIdx.x; sid < nslots; sid += stride) {
        const int row = sid / slots_per_row;
        const int slot = sid - row * slots_per_row;
        const int x = slot * 16;
        unsigned b16 = 0;
        if (x < W) {
            const uint4 v = *reinterpret_cast<const uint4*>(fm + (size_t)row * W + x);
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                b16 |= ((w4[q] & 0x000000ffu) ? 1u : 0u) << (4 * q);
                b16 |= ((w4[q] & 0x0000ff00u) ? 2u : 0u) << (4 * q);
                b16 |= ((w4[q] & 0x00ff0000u) ? 4u : 0u) << (4 * q);
                b16 |= ((w4[q] & 0xff000000u) ? 8u : 0u) << (4 * q);
            }
        }
        if (mf) acc.add(b16, x, row, H, W);   // (the lane's own 16 pixels: no wait for the shuffles)
        unsigned long long word = (unsigned long long)b16 << (16 * (slot & 3));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        if ((slot & 3) == 0) fb[(size_t)row * WW + (slot >> 2)] = word;
    }
    if (mf) lg_box_flush(acc, s_box, mf + (size_t)frame * LG_MF);
}

// blocks per frame of a (blocks, B) grid of 256-thread workgroups over `units` threads' worth of work per frame: about `target`
// workgroups in all, as the one-dimensional grids these kernels had
static unsigned lg_pack_blocks(long long units, int B, long long target) {
    const long long full = (units + 255) / 256;
    return (unsigned)std::max<long long>(1, std::min<long long>(full, target / B));
}

void lg_launch_pack_bits(const uint8_t* mask, unsigned long long* bits, int B, int H, int W, int WW, hipStream_t s, uint32_t* mf) {
    if ((W & 15) == 0 && ((uintptr_t)mask & 15) == 0) {
        hipLaunchKernelGGL(lg_pack_bits16_kernel, dim3(lg_pack_blocks((long long)H * WW * 4, B, 16384), B), dim3(256), 0, s, mask, bits,
                           H, W, WW, mf);
        return;
    }
    hipLaunchKernelGGL(lg_pack_bits_kernel, dim3(lg_pack_blocks((long long)H * WW * 64, B, 8192), B), dim3(256), 0, s, mask, bits, H, W,
                       WW, mf);
}

// The node's `optimal_mask = mask_tensor == optimal_leaf_id` (leaf_grasp_node_v3.py:118) folded into the bit-row pass: labels
// [B][H][W] int16 and one leaf id per frame in, the 0 / 1 byte mask (what the sweeps and the patch gather read) and the bit rows
// out.  One pass over the labels instead of torch's comparison (labels in, mask out) + lg_pack_bits (mask in).  A lane takes 16
// labels (two 16-byte loads), four adjacent lanes assemble a word; W % 16 == 0 (the launcher falls back otherwise).
// OTHERS (label-aware mode; false: the code as it was, the two extra arguments unused): the same labels also give the bit rows
// of the other leaves, label > 0 && label != id, and the frame's "has another leaf" word (iso_mf[.. + 2], one atomic per wave
// that saw one).
template <bool OTHERS>
__global__ __launch_bounds__(256) void lg_pack_labels16_kernel(const int16_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                               uint8_t* __restrict__ mask, unsigned long long* __restrict__ bits,
                                                               int H, int W, int WW, uint32_t* __restrict__ mf,
                                                               unsigned long long* __restrict__ others, uint32_t* __restrict__ iso_mf) {
    __shared__ uint32_t s_box[5];
    const int slots_per_row = 4 * WW, frame = blockIdx.y;
    const int nslots = H * slots_per_row;                        // of one frame; a multiple of 4
    const int16_t* fl = labels + (size_t)frame * H * W;
    uint8_t* fm = mask + (size_t)frame * H * W;
    unsigned long long* fb = bits + (size_t)frame * H * WW;
    const int id = ids[frame];
    LgBoxAcc acc;
    unsigned o_any = 0;
    const int stride = gridDim.x * 256;  // multiple of 4: a word's four slots stay in adjacent lanes
    for (int sid = blockIdx.x * 256 + threadIdx.x; sid < nslots; sid += stride) {
        const int row = sid / slots_per_row;
        const int slot = sid - row * slots_per_row;
        const int x = slot * 16;
        unsigned b16 = 0, o16 = 0;
        if (x < W) {
            const uint4 v0 = *reinterpret_cast<const uint4*>(fl + (size_t)row * W + x);
            const uint4 v1 = *reinterpret_cast<const uint4*>(fl + (size_t)row * W + x + 8);
            const uint32_t w8[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            uint32_t mb[4];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned lo = (int)(int16_t)(w8[q] & 0xffffu) == id ? 1u : 0u, hi = (int)(int16_t)(w8[q] >> 16) == id ? 1u : 0u;
                b16 |= (lo | (hi << 1)) << (2 * q);
                if constexpr (OTHERS) {
                    const int l0 = (int)(int16_t)(w8[q] & 0xffffu), l1 = (int)(int16_t)(w8[q] >> 16);
                    o16 |= ((l0 > 0 && l0 != id ? 1u : 0u) | (l1 > 0 && l1 != id ? 2u : 0u)) << (2 * q);
                }
                const uint32_t two = lo | (hi << 8);
                if (q & 1) mb[q >> 1] |= two << 16; else mb[q >> 1] = two;
            }
            *reinterpret_cast<uint4*>(fm + (size_t)row * W + x) = make_uint4(mb[0], mb[1], mb[2], mb[3]);
        }
        if (mf) acc.add(b16, x, row, H, W);
        unsigned long long word = (unsigned long long)b16 << (16 * (slot & 3));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        if ((slot & 3) == 0) fb[(size_t)row * WW + (slot >> 2)] = word;
        if constexpr (OTHERS) {
            unsigned long long ow = (unsigned long long)o16 << (16 * (slot & 3));
            ow |= __shfl_xor(ow, 1, 64);
            ow |= __shfl_xor(ow, 2, 64);
            if ((slot & 3) == 0) others[((size_t)frame * H + row) * WW + (slot >> 2)] = ow;
            o_any |= o16;
        }
    }
    if (mf) lg_box_flush(acc, s_box, mf + (size_t)frame * LG_MF);
    if constexpr (OTHERS) {
        if (__ballot(o_any != 0) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&iso_mf[(size_t)frame * LG_ISO_MF + 2], 1u);
    }
}
__global__ __launch_bounds__(256) void lg_labels_mask_kernel(const int16_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                             uint8_t* __restrict__ mask, long long px_per_frame, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        mask[i] = (int)labels[i] == ids[i / px_per_frame] ? 1 : 0;
}
void lg_launch_pack_labels(const int16_t* labels, const int32_t* ids_dev, uint8_t* mask, unsigned long long* bits, int B, int H,
                           int W, int WW, hipStream_t s, uint32_t* mf, unsigned long long* others, uint32_t* iso_mf) {
    if ((W & 15) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)mask & 15) == 0) {
        const dim3 grid(lg_pack_blocks((long long)H * WW * 4, B, 16384), B);
        if (others)
            hipLaunchKernelGGL(lg_pack_labels16_kernel<true>, grid, dim3(256), 0, s, labels, ids_dev, mask, bits, H, W, WW, mf, others, iso_mf);
        else
            hipLaunchKernelGGL(lg_pack_labels16_kernel<false>, grid, dim3(256), 0, s, labels, ids_dev, mask, bits, H, W, WW, mf,
                               (unsigned long long*)nullptr, (uint32_t*)nullptr);
        return;
    }
    if (others) lg_launch_pack_others(labels, ids_dev, others, iso_mf, B, H, W, WW, s);
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(lg_labels_mask_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 16384)), dim3(256), 0, s, labels,
                       ids_dev, mask, (long long)H * W, total);
    lg_launch_pack_bits(mask, bits, B, H, W, WW, s, mf);
}

// Export of the bits the host needs -- the rows and 64-bit words of each frame's bounding box only (a leaf spans a third
// of the frame in each direction: ~10x less PCIe traffic than the whole batch) -- by posted 8-byte writes into the pinned host image,
// which keeps its [B][H][WW] layout; rows outside the bounding box are all zero and never read by the host.
__global__ __launch_bounds__(256) void lg_export_rows_kernel(const unsigned long long* __restrict__ bits,
                                                             const LgWin* __restrict__ wins,
                                                             unsigned long long* __restrict__ dst_host, int H, int WW) {
    const int frame = blockIdx.y;
    const LgWin w = wins[frame];
    if (w.bx1 < w.bx0) return;
    const int w0 = w.bx0 >> 6, nw = (w.bx1 >> 6) - w0 + 1;          // words of the bounding box
    const size_t base = ((size_t)frame * H + w.by0) * WW + w0;
    const long long n = (long long)(w.by1 - w.by0 + 1) * nw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const size_t o = base + (size_t)(i / nw) * WW + (size_t)(i % nw);
        dst_host[o] = bits[o];
    }
}

void lg_launch_export_rows(const unsigned long long* bits, const LgWin* wins, unsigned long long* dst_host_devptr, int B,
                           int H, int WW, hipStream_t s) {
    hipLaunchKernelGGL(lg_export_rows_kernel, dim3(2, B), dim3(256), 0, s, bits, wins, dst_host_devptr, H, WW);
}

// ============================================================================ stem penalty (binary dilation on bit rows)
// stem = dilate(mask & bottom_region, ellipse k) & mask     (grasp_point_selector.py:688-701)
// The per-word code is in lg_internal.h (lg_stem_word_rows, lg_stem_word_chain).
// Per-row form, one thread per (frame, y, word): the fallback for spans that are not nested, and the A/B arm (LG_STEM_ALGO=0).
__global__ __launch_bounds__(256) void lg_stem_bits_kernel(const unsigned long long* __restrict__ bits,
                                                           unsigned long long* __restrict__ stem, int H, int W, int WW,
                                                           int bottom_start, LgSeSpans se) {
    long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    long long per_frame = (long long)H * WW;
    int b = blockIdx.y;
    if (gid >= per_frame) return;
    int y = (int)(gid / WW), w = (int)(gid % WW);
    const unsigned long long* fb = bits + (long long)b * per_frame;
    unsigned long long self = fb[(long long)y * WW + w];
    unsigned long long acc = 0;
    if (self != 0 && y + (se.n - 1 - se.anchor) >= bottom_start) acc = lg_stem_word_rows(fb, H, WW, bottom_start, y, w, se);
    stem[(long long)b * per_frame + gid] = acc & self;
}

// Nested-span form.  gridDim.x workgroups per frame: first every word outside the frame's active rectangle (lg_stem_active) is
// zeroed by its index alone, without a load -- the whole plane is written on every call, lg_final_kernel reads whole tile rows
// and a small leaf after a large one must not meet stale words -- then the words of the rectangle, mapped densely onto the
// threads, do the arithmetic.  A frame whose bounding box lies above the ellipse's reach does none.
__global__ __launch_bounds__(256) void lg_stem_chain_kernel(const unsigned long long* __restrict__ bits,
                                                            unsigned long long* __restrict__ stem,
                                                            const LgWin* __restrict__ wins, int H, int WW, int bottom_start,
                                                            LgSeSpans se, LgStemPlan plan) {
    const int b = blockIdx.y;
    const size_t per_frame = (size_t)H * WW;
    const unsigned long long* fb = bits + (size_t)b * per_frame;
    unsigned long long* fs = stem + (size_t)b * per_frame;
    const LgStemRect rc = lg_stem_active(wins[b], H, WW, bottom_start, se.n, se.anchor);
    const int ya = rc.ya, yb = rc.yb, w0 = rc.w0, w1 = rc.w1;
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    for (int i = tid; i < (int)per_frame; i += nth) {   // (H * WW <= 16384 * 128)
        const int y = i / WW, w = i - y * WW;
        if (!(y >= ya && y <= yb && w >= w0 && w <= w1)) fs[i] = 0ull;
    }
    if (ya > yb) return;
    const int nw = w1 - w0 + 1, nact = (yb - ya + 1) * nw;
    for (int i = tid; i < nact; i += nth) {
        const int r = i / nw, y = ya + r, w = w0 + (i - r * nw);
        const size_t o = (size_t)y * WW + w;
        const unsigned long long self = fb[o];
        fs[o] = self ? (lg_stem_word_chain(fb, H, WW, bottom_start, y, w, se, plan) & self) : 0ull;
    }
}

void lg_launch_stem_bits(const unsigned long long* bits, unsigned long long* stem, const LgWin* wins, int B, int H, int W, int WW,
                         int bottom_start, const LgSeSpans& se, const LgStemPlan* plan, hipStream_t s) {
    long long per_frame = (long long)H * WW;
    if (plan && plan->nested && wins) {
        // eight words of the plane per thread, at most 16 workgroups per frame (256 frames of 1080p: 4096 workgroups)
        const unsigned nblk = (unsigned)std::max<long long>(1, std::min<long long>((per_frame + 2047) / 2048, 16));
        hipLaunchKernelGGL(lg_stem_chain_kernel, dim3(nblk, B), dim3(256), 0, s, bits, stem, wins, H, WW, bottom_start, se, *plan);
        return;
    }
    dim3 grid((unsigned)((per_frame + 255) / 256), B);
    hipLaunchKernelGGL(lg_stem_bits_kernel, grid, dim3(256), 0, s, bits, stem, H, W, WW, bottom_start, se);
}

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
__device__ __forceinline__ float lg_uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// ---- the per-pixel arithmetic, stated once: lg_final_kernel and the deferred form of lg_gather_kernel both call these, so a
//      plane the gather computes at its windows is the float the plane kernel would have stored there.  hipcc contracts a * b + c
//      to an FMA where it likes, and the same inlined source did not contract alike in two kernels (sdf and the gradient's square
//      came out with the other product fused): contraction is therefore off in lg_flat4 and lg_pixels4 and every FMA is written
//      out -- in the form the plane kernel has been compiled to all along, so its planes keep their bits.
//      FROZEN HISTORY, NOT A NUMERICAL CHOICE: which product is fused where (pixel 0 of four unfused, f^2 fused for pixels 0-1,
//      FUSE_SY by instantiation) is what one compiler version happened to emit for the plane kernel before these functions
//      existed.  No form is more accurate than another; they are written down so that the planes, the patches and every test
//      that compares them byte for byte stay what they were.  Do not tidy them up.  The Gaussian taps below are NOT pinned
//      (see there): a toolchain change can still alter the last bit of flatness, in every kernel alike.
// Gaussian taps in ascending order, along a row (stride 1) and down a column (stride S floats)
// (These two stay under the compiler's contraction: inside lg_final_kernel's unrolled row loops it compiles them to a mixture of
// packed multiplies + adds and FMAs that depends on the row's place in the tile.  The smoothed plane, and with it flatness, can
// therefore not be recomputed bit for bit anywhere else without changing the plane kernel's own output: flatness stays a
// stored plane, profiles/NOTES_deferred_planes.md.)
template <int R>
__device__ __forceinline__ float lg_tap_row(const float (&kw)[2 * R + 1], const float* p) {
    float acc = kw[0] * p[0];
#pragma unroll
    for (int i = 1; i < 2 * R + 1; i++) acc += kw[i] * p[i];
    return acc;
}
template <int R, int S>
__device__ __forceinline__ float lg_tap_col(const float (&kw)[2 * R + 1], const float* p) {
    float acc = kw[0] * p[0];
#pragma unroll
    for (int i = 1; i < 2 * R + 1; i++) acc += kw[i] * p[i * S];
    return acc;
}
// flatness of four pixels x .. x + 3 of a row: Sobel cross-correlation on the smoothed, reflect-padded plane, exp(-scale |grad|)
// (:646-655).  ga, gb, gc: rows y - 1, y, y + 1 of that plane at columns x - 1 .. x + 4.  (2 * g is exact: the sums round the
// same fused or not.)  FUSE_SY: which square of sx^2 + sy^2 is fused -- the instantiations of the plane kernel had been compiled
// either way: every plane wanted and W % 4 == 0 fused sy, the others sx; the score-only form follows the dense call of its width.
template <bool FUSE_SY>
__device__ __forceinline__ void lg_flat4(const float (&ga)[6], const float (&gb)[6], const float (&gc)[6], float flat_scale,
                                         float (&o_flat)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float sx = (ga[j + 2] - ga[j]) + 2.0f * (gb[j + 2] - gb[j]) + (gc[j + 2] - gc[j]);
        float sy = (gc[j] + 2.0f * gc[j + 1] + gc[j + 2]) - (ga[j] + 2.0f * ga[j + 1] + ga[j + 2]);
        const float g2 = FUSE_SY ? __builtin_fmaf(sy, sy, sx * sx) : __builtin_fmaf(sx, sx, sy * sy);
        o_flat[j] = __expf(-flat_scale * __builtin_amdgcn_sqrtf(g2));  // v_sqrt_f32, 1 ulp
    }
}
// frame scalars of the per-pixel block.  AP: a pointer to the LgFinalArgs (the plane kernel's kernarg segment, or the
// gather's by-value copy); FP / MP: the frame's LgFrameParams and its two maxfix words
struct LgPixFrame {
    int has_angle;
    float sin_t, cos_t, inv_maxabs, opt_d, inv_2s2, focal, f2, ramp_step;
};
template <class AP, class FP, class MP>
__device__ __forceinline__ LgPixFrame lg_pix_frame(AP ap, FP fpp, MP mfp) {
    LgPixFrame c;
    c.has_angle = fpp->has_angle;
    c.sin_t = fpp->sin_t; c.cos_t = fpp->cos_t;
    const uint32_t mfi = mfp[0], mfo = mfp[1];
    const float maxabs = fmaxf((float)mfi * (1.0f / 65536.0f), (float)mfo * (1.0f / 65536.0f));
    c.inv_maxabs = lg_uniform_f(__frcp_rn(maxabs));
    c.opt_d = ap->optimal_distance;
    c.inv_2s2 = ap->inv_2s2;
    c.focal = ap->f;
    c.f2 = c.focal * c.focal;
    c.ramp_step = ap->iso_ramp_step;
    return c;
}
// the four pixels x0 .. x0 + 3 of row y on a wave that holds a leaf pixel: geometry, SDF / edge term, isolation (ISO: it is no
// part of `traditional`, the score-only plane kernel leaves it out), fusion, validity.  mnib / snib: their mask and stem bits;
// din: distance_map; o_flat: lg_flat4.  Returns the validity bytes (bit 8 j: pixel j).
// Which products are fused is the plane kernel's compiled form, by the pixel's place x & 3 in its lane's four (x0 % 4 == 0
// there; the gather's groups start anywhere): pixel 0 rounds dx^2 and dy^2 separately (they were one packed multiply), pixels
// 1-3 fuse dx^2; pixels 0-1 fuse f^2 into r^2 + f^2, pixels 2-3 add the rounded f^2.
template <bool ISO, class AP>
__device__ __forceinline__ uint32_t lg_pixels4(AP ap, const LgPixFrame& c, int y, int x0, int H, int W, unsigned mnib, unsigned snib,
                                               const float* din, const float (&o_flat)[4], float w_flat, float (&o_sdf)[4],
                                               float (&o_app)[4], float (&o_iso)[4], float (&o_acc)[4], float (&o_stem)[4],
                                               float (&o_trad)[4], bool (&o_valid)[4]) {
#pragma clang fp contract(off)
    uint32_t vbytes = 0;
    const float dyp = (float)(y - ap->cyi) - ap->cyf;  // exact integer part first: no cancellation near the centre
    const float dyp2 = dyp * dyp;
    const int dyb = min(y + 1, H - y);
    const float ramp = __builtin_fmaf(c.ramp_step, (float)y, ap->iso_ramp_top);
    const float w_approach = ap->w_approach, w_sdf = ap->w_sdf, w_access = ap->w_access;
    const int has_angle = c.has_angle;
    const float sin_t = c.sin_t, cos_t = c.cos_t, inv_maxabs = c.inv_maxabs, opt_d = c.opt_d, inv_2s2 = c.inv_2s2;
    const float focal = c.focal, f2 = c.f2;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = x0 + j;
        const float m = ((mnib >> j) & 1u) ? 1.0f : 0.0f;
        const float st = ((snib >> j) & 1u) ? 1.0f : 0.0f;
        // closed-form geometry planes                                           (:502-524, :569-593)
        const float dxp = (float)(x - ap->cxi) - ap->cxf;
        const int jj = x & 3;
        const float r2 = jj == 0 ? dxp * dxp + dyp2 : __builtin_fmaf(dxp, dxp, dyp2);
        const float inv_r = r2 > 0.0f ? rsqrtf(r2) : 0.0f;
        const float r = r2 * inv_r;
        const float r2f2 = jj < 2 ? __builtin_fmaf(focal, focal, r2) : f2 + r2;
        const float app = focal * rsqrtf(r2f2) * m;
        const float cosang = r2 > 0.0f ? dxp * inv_r : 1.0f;
        const float acc = __builtin_fmaf(ap->access_w_dir, cosang, ap->access_w_dist * __builtin_fmaf(-ap->inv_maxd, r, 1.0f)) * m;
        // SDF / edge term                                                        (:526-567)
        const float align = has_angle ? fabsf(__builtin_fmaf(sin_t, dxp * inv_r, -(cos_t * (dyp * inv_r)))) : 1.0f;
        const float dd = din[j] - opt_d;
        const float interior = __expf(-(dd * dd) * inv_2s2);
        const float sdfn = din[j] * inv_maxabs;  // inside the mask d_out == 0
        const float sdf = __builtin_fmaf(ap->sdf_w_sdf, sdfn, __builtin_fmaf(ap->sdf_w_interior, interior, ap->sdf_w_align * align)) * m;
        float iso = 0.0f;
        if (ISO) {
            // degenerate isolation map: chamfer-3 transform of an image with no zero pixel (:595-633)
            const int dbrd = min(min(x + 1, W - x), dyb);
            const float dt3 = (float)(ap->init0 + (uint32_t)dbrd * LG_A3) * (1.0f / 65536.0f);
            const float s = dt3 * ap->iso_inv_max;
            iso = __builtin_fmaf(ap->iso_w_close, s, ap->iso_w_wide * s) * ramp * m;
        }
        // fusion + validity                                                      (:272-288)
        const float trad = __builtin_fmaf(w_access, acc, __builtin_fmaf(w_flat, o_flat[j], __builtin_fmaf(w_approach, app, w_sdf * sdf))) *
                           (1.0f - st);
        const bool valid = (din[j] > ap->min_edge_distance) && (m > 0.0f) && (st < ap->stem_valid_thresh);
        o_sdf[j] = sdf; o_app[j] = app; o_iso[j] = iso; o_acc[j] = acc; o_stem[j] = st; o_trad[j] = trad;
        o_valid[j] = valid;
        if (valid) vbytes |= 1u << (8 * j);
    }
    return vbytes;
}

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
        li = xcd_first + it;
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

// ============================================================================ the tail of select_grasp_point, per frame
// grasp_point_selector.py:205-245 after the candidates exist: CNN rescoring (ml = tanh(3 sigmoid(logit)) / 2 + 1/2, confidence
// weights, "take it if the combined score beats the best so far", :210-237), get_3d_grasp_point (:152-180) and
// calculate_pre_grasp_point (:754-819: five probes of the leaf mask dilated by the clearance ellipse along the viewing ray,
// fallback at 0.10 m).  One wave per frame; the same float64 operations in the same order as the host code this replaces (fp
// contraction off), the selection loop sequential in lane 0 -- the call no longer ships candidate lists, logits and bit rows to
// the host and walks the frames there (0.1 ms of host work + five copies per 256-frame call, with the GPU idle behind them).
// CNN rescoring of candidate i of frame b (:210-237): ml = get_ml_score's tanh(3 sigmoid(logit)) / 2 + 1/2 (:133-136), its
// confidence (:222), weight (:223) and combined score (:226).  false: a border candidate of a torch.bool mask has no ML score
// (SURVEY App. B.7).  lg_finish_kernel and lg_candidates_kernel both call this.
__device__ inline bool lg_ml_rescore(const LgFinishArgs& a, int b, int i, int x, int y, double trad, double* ml_out,
                                     double* conf_out, double* comb_out) {
#pragma clang fp contract(off)
    if (a.mask_is_bool && (x < 16 || y < 16 || x + 16 > a.W || y + 16 > a.H)) return false;
    // (a.slot: the CNN ran on the survivors only; a candidate that cannot beat candidate 0 has no patch and is never taken)
    int j = b * a.K + i;
    if (a.slot) {
        j = a.slot[j];
        if (j < 0) return false;
        j += (b / a.slot_frames) * a.slot_frames * a.K;
    }
    lg_ml_combine((double)a.logits[j], trad, ml_out, conf_out, comb_out);
    return true;
}

struct LgPoint3d { float X, Y, Z; int has_pre; float pX, pY, pZ; };

// get_3d_grasp_point (:152-180) of pixel (x, y) at depth Z and calculate_pre_grasp_point (:754-819): five probes of the leaf
// mask dilated by the clearance ellipse along the viewing ray, fallback at 0.10 m.  Called by every lane of ONE wave with the
// same arguments (lane i tests row i of the structuring element; __ballot): every lane gets the same result.
__device__ inline LgPoint3d lg_point_3d_pre(const LgFinishArgs& a, int b, int x, int y, double Z, int lane) {
#pragma clang fp contract(off)
    const int H = a.H, W = a.W, WW = a.WW;
    LgPoint3d R;
    R.has_pre = 0; R.pX = 0.f; R.pY = 0.f; R.pZ = 0.f;
    const double X = Z * ((double)x - a.cx) / a.f;
    const double Y = Z * ((double)y - a.cy) / a.f;
    R.X = (float)X; R.Y = (float)Y; R.Z = (float)Z;
    const double nrm = sqrt(X * X + Y * Y + Z * Z);
    if (!(nrm > 0.0) || !isfinite(nrm)) return R;    // reference: exception -> None
    const double dxn = X / nrm, dyn = Y / nrm;
    const unsigned long long* fb = a.bits + (size_t)b * H * WW;
    const unsigned long long* fb2 = a.bits2 ? a.bits2 + (size_t)b * H * WW : nullptr;   // label-aware mode: the other leaves
    bool done = false;
    for (int step = 0; step < 5 && !done; step++) {
        // np.arange(0.05, 0.10, 0.01)[step] = start + step * ((start + delta) - start)
        const double dist = 0.05 + (double)step * ((0.05 + 0.01) - 0.05);
        const double tx = X - dxn * dist, ty = Y - dyn * dist, tz = Z;
        const int u = (int)((tx * a.f / tz) + a.cx);
        const int v = (int)((ty * a.f / tz) + a.cy);
        if (!(u >= 0 && u < W && v >= 0 && v < H)) continue;
        // dilated[v, u] != 0  <=>  some set pixel under the ellipse centred there: lane i tests row i of the structuring element
        bool hit = false;
        if (lane < a.se.n && a.se.lo[lane] <= a.se.hi[lane]) {
            const int yy = v + lane - a.se.anchor;
            const int x0 = max(u + a.se.lo[lane], 0), x1 = min(u + a.se.hi[lane], W - 1);
            if (yy >= 0 && yy < H && x0 <= x1) {
                const unsigned long long* row = fb + (size_t)yy * WW;
                for (int w = x0 >> 6; w <= (x1 >> 6); w++) {
                    unsigned long long m = ~0ull;
                    if (w == (x0 >> 6)) m &= ~0ull << (x0 & 63);
                    if (w == (x1 >> 6)) m &= ~0ull >> (63 - (x1 & 63));
                    hit |= (row[w] & m) != 0ull;
                    if (fb2) hit |= (fb2[(size_t)yy * WW + w] & m) != 0ull;
                }
            }
        }
        if (__ballot(hit) == 0ull) {
            const double dg = sqrt((tx - X) * (tx - X) + (ty - Y) * (ty - Y));
            if (dg >= 0.05) { R.pX = (float)tx; R.pY = (float)ty; R.pZ = (float)tz; done = true; }
        }
    }
    if (!done) { R.pX = (float)(X - dxn * 0.10); R.pY = (float)(Y - dyn * 0.10); R.pZ = (float)Z; }
    R.has_pre = 1;
    return R;
}

__global__ __launch_bounds__(64) void lg_finish_kernel(LgFinishArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_comb[64];
    __shared__ int s_elig[64], s_best, s_ml;
    __shared__ double s_bs;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.cand_n[b], K = a.K;
    lg_grasp_result R;
    R.found = 0; R.x = 0; R.y = 0; R.X = 0.f; R.Y = 0.f; R.Z = 0.f; R.has_pre = 0; R.pX = 0.f; R.pY = 0.f; R.pZ = 0.f;
    R.n_candidates = n; R.ml_used = 0; R.best_score = 0.f; R.theta = a.fp[b].theta;
    if (n <= 0) {   // reference: "No valid candidate points found" -> (None, None, None)
        if (lane == 0) a.out[b] = R;
        return;
    }
    const int32_t* xy = a.cand_xy + (size_t)b * K * 2;
    const float* info = a.cand_info + (size_t)b * K * 2;
    const bool rescoring = a.use_cnn && n > 1;
    double comb = 0.0, ml, conf;
    int elig = 0;
    if (rescoring && lane < n)
        elig = lg_ml_rescore(a, b, lane, xy[2 * lane], xy[2 * lane + 1], (double)info[2 * lane], &ml, &conf, &comb) ? 1 : 0;
    s_comb[lane] = comb;
    s_elig[lane] = elig;
    __syncthreads();
    if (lane == 0) {
        int best = 0, ml_used = 0;
        double best_score = (double)info[0];  // candidate 0's traditional score (:205-206)
        if (rescoring)
            for (int i = 0; i < n; i++)
                if (s_elig[i] && s_comb[i] > best_score) { best_score = s_comb[i]; best = i; ml_used = 1; }
        s_best = best; s_ml = ml_used; s_bs = best_score;
    }
    __syncthreads();
    const int best = s_best;
    R.found = 1;
    R.ml_used = s_ml;
    R.x = xy[2 * best]; R.y = xy[2 * best + 1];
    R.best_score = (float)s_bs;
    const LgPoint3d g = lg_point_3d_pre(a, b, R.x, R.y, (double)info[2 * best + 1], lane);
    R.X = g.X; R.Y = g.Y; R.Z = g.Z;
    R.has_pre = g.has_pre; R.pX = g.pX; R.pY = g.pY; R.pZ = g.pZ;
    if (lane == 0) a.out[b] = R;
}

void lg_launch_finish(const LgFinishArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lg_finish_kernel, dim3(a.B), dim3(64), 0, s, a);
}

// ============================================================================ every candidate, ranked
// One workgroup per frame.  Lanes compute each candidate's ML fields (lg_ml_rescore: the operations lg_finish_kernel runs);
// then lane 0 of wave 0 ranks them (lg_rank_candidates, the host export's code) while waves 1.. compute each candidate's 3-D
// and pre-grasp point, one wave per candidate (lg_point_3d_pre; the point does not depend on the rank, so the two overlap);
// then the rows are written in rank order from LDS.  Rows past n get index -1 and zeros.  Rank 0 is lg_finish_kernel's row.
// (Measured: four waves that each took the ranks wave, wave + 4, ... after the ranking: 0.053 ms per launch at any B.)
#define LG_CAND_WAVES 16
__global__ __launch_bounds__(64 * LG_CAND_WAVES) void lg_candidates_kernel(LgFinishArgs a, lg_grasp_candidate* __restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double s_trad[64], s_comb[64], s_ml[64], s_conf[64], s_pick[64];
    __shared__ int32_t s_scored[64], s_order[64], s_by[64];
    __shared__ LgPoint3d s_pt[64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int K = a.K, n = min(a.cand_n[b], K);
    const int32_t* xy = a.cand_xy + (size_t)b * K * 2;
    const float* info = a.cand_info + (size_t)b * K * 2;
    const bool rescoring = a.use_cnn && n > 1;
    if (t < n) {
        const double tr = (double)info[2 * t];
        double ml = __builtin_nan(""), conf = __builtin_nan(""), comb = __builtin_nan("");
        const bool sc = rescoring && lg_ml_rescore(a, b, t, xy[2 * t], xy[2 * t + 1], tr, &ml, &conf, &comb);
        s_trad[t] = tr; s_comb[t] = comb; s_ml[t] = ml; s_conf[t] = conf;
        s_scored[t] = sc ? 1 : 0;
    }
    __syncthreads();
    if (wave == 0) {
        if (lane == 0) lg_rank_candidates(s_trad, s_comb, s_scored, n, rescoring ? 1 : 0, s_order, s_pick, s_by);
    } else {
        for (int i = wave - 1; i < n; i += LG_CAND_WAVES - 1) {   // wave-uniform: lg_point_3d_pre ballots across the wave
            const LgPoint3d g = lg_point_3d_pre(a, b, xy[2 * i], xy[2 * i + 1], (double)info[2 * i + 1], lane);
            if (lane == 0) s_pt[i] = g;
        }
    }
    __syncthreads();
    lg_grasp_candidate* out = rows + (size_t)b * K;
    for (int r = t; r < K; r += 64 * LG_CAND_WAVES) {
        lg_grasp_candidate R;
        memset(&R, 0, sizeof(R));
        R.index = -1;
        if (r < n) {
            const int i = s_order[r];
            R.index = i;
            R.x = xy[2 * i]; R.y = xy[2 * i + 1];
            R.traditional = info[2 * i];
            R.ml_score = (float)s_ml[i]; R.ml_confidence = (float)s_conf[i]; R.combined = (float)s_comb[i];
            R.scored = s_scored[i];
            R.pick_score = (float)s_pick[r];
            R.by_ml = s_by[r];
            const LgPoint3d g = s_pt[i];
            R.X = g.X; R.Y = g.Y; R.Z = g.Z;
            R.has_pre = g.has_pre; R.pX = g.pX; R.pY = g.pY; R.pZ = g.pZ;
        }
        out[r] = R;
    }
}

void lg_launch_candidates(const LgFinishArgs& a, lg_grasp_candidate* rows, hipStream_t s) {
    hipLaunchKernelGGL(lg_candidates_kernel, dim3(a.B), dim3(64 * LG_CAND_WAVES), 0, s, a, rows);
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
