// Mask and labels to bit rows (with every frame's bounding box and area), the bounding-box export, and the stem bits.
// Reference semantics: scripts/utils/grasp_point_selector.py (cited per kernel); design: DESIGN.md.
#include "lg_bits.h"
#include "lg_iso.h"
#include "lg_wave.h"

#include <algorithm>

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
// The per-word code is in lg_bits.h (lg_stem_word_rows, lg_stem_word_chain).
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
