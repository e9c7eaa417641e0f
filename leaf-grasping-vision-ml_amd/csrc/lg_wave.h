// Wave- and workgroup-level device helpers that more than one HIP translation unit of liblgrasp.so needs (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt(0), which would stall
// every image row of the distance-transform sweeps on its own global prefetch (rows are ~1000 cycles apart,
// HBM latency is longer): LDS operations are complete at lgkmcnt(0), global loads/stores stay in flight.
__device__ __forceinline__ void lg_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ uint32_t lg_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        uint32_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
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
