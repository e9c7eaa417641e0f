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
