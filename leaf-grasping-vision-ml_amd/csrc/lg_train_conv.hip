// Training step, convolutions: forward, backward-data and backward-weights of the encoder's 3x3 layers, the weight repacking
// they read, and their launchers (lg_train.h).
//
// The convolutions run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation) as implicit GEMMs whose operands
// are gathered per lane from an LDS-staged halo tile:
//   forward / backward-data : M = output channel, N = pixel, K = (tap, input channel)
//   backward-weights        : M = input channel,  N = output channel, K = pixel, one accumulator per tap; split over
//                             pixel tiles into partial sums that a second kernel adds in a fixed order (deterministic).
// The pixel index runs over (sample, y, x), so small feature maps (8x8, 4x4) fill a tile with several samples.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lg_train.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ float lgt_zero_pad[4];// zero-initialised source for padded / out-of-range direct-to-LDS lanes

namespace {

// ------------------------------------------------------------------------------------------------ tiles
template <int WI, int TILE>
struct Tile {
    static constexpr int HW = WI * WI;
    static constexpr int TS = HW >= TILE ? 1 : TILE / HW;   // samples per tile
    static constexpr int TR = HW >= TILE ? TILE / WI : WI;  // image rows per tile
    static constexpr int BANDS = WI / TR;
    static constexpr int TW = WI + 2, TH = TR + 2;          // staged rows / columns (halo 1)
    static constexpr int PLANE = TS * TH * TW;              // staged floats per channel
    __device__ static constexpr int halo(int q) {           // offset of the 3x3 window's top-left for tile pixel q
        const int ts = q / (TR * WI), row = (q / WI) % TR, x = q % WI;
        return (ts * TH + row) * TW + x;
    }
};

// ------------------------------------------------------------------------------------------------ conv fwd / dgrad
// out[n][co][y][x] = bias[co] + sum_{tap,ci} wp[tap][ci][co] * in[n][ci][y+ky-1][x+kx-1]     (zero padding)
// Workgroup = 4 waves = WPX x WCO x KS waves over (pixels, output channels, slices of the staged input channels); a wave
// owns PB x CB blocks of 32 pixels x 32 channels.  Three shapes:
//   <PB 2, CB 2, WPX 4, KS 1>  256 pixels x 64 channels, 4 MFMAs per 4 LDS operand reads   -- large batches
//   <PB 1, CB 1, WPX 2, KS 1>   64 pixels x 64 channels, 4x the workgroups                  -- small batches
//   <PB 1, CB 1, WPX 1, KS 4>   32 pixels x 32 channels, the four waves split K             -- the reference's batch of 16,
//                                where a 8x8 layer has 1024 pixels in total: 256 workgroups instead of 16
template <int WI, int PB, int CB, int WPX, int KS, int KC>
__global__ __launch_bounds__(256) void lgt_conv_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                       const float* __restrict__ bias, float* __restrict__ out, int N,
                                                       int CI, int CO) {
    constexpr int WCO = 4 / (WPX * KS), TILE = 32 * PB * WPX, COT = 32 * CB * WCO, KCT = KC * KS;
    static_assert(WPX * WCO * KS == 4, "4 waves");
    using T = Tile<WI, TILE>;
    constexpr int IN_ELEMS = KCT * T::PLANE, NIN = (IN_ELEMS + 255) / 256, IN_PAD = NIN * 256;
    constexpr int W4_ELEMS = 9 * KCT * (COT / 4), NW4 = (W4_ELEMS + 255) / 256;
    constexpr int BUF = IN_PAD + NW4 * 1024;   // floats per stage
    // one shared object, two stages of [input halo tile | weights], both filled by global_load_lds in load order
    __shared__ __attribute__((aligned(16))) float s_buf[2 * BUF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 31, kh = lane >> 5;
    const int wpx = wave % WPX, wco = (wave / WPX) % WCO, ks = wave / (WPX * WCO);
    const int tile = blockIdx.x, n0 = (tile / T::BANDS) * T::TS, y0 = (tile % T::BANDS) * T::TR, co0 = blockIdx.y * COT;

    f32x16 acc[PB][CB];
#pragma unroll
    for (int i = 0; i < PB; i++)
#pragma unroll
        for (int j = 0; j < CB; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
    int boff[PB];
#pragma unroll
    for (int i = 0; i < PB; i++) boff[i] = T::halo((wpx * PB + i) * 32 + lm);
    const int aoff = wco * CB * 32 + lm;

    // Direct-to-LDS staging: chunk c+1 streams into the other stage while the MFMA loop works on chunk c.  The LDS
    // destination of one wave instruction is a wave-uniform base + lane * size, i.e. slot idx = t + 256 j lands at
    // float idx (input) / float4 idx (weights): the images are linear in idx.  Zero padding of the convolution, channels
    // past CI / CO and unused slots are fetched from a zeroed device word.  Source offsets are chunk-invariant apart from
    // the channel base and computed once.
    int off_in[NIN], ci_in[NIN], off_w[NW4], ci_w[NW4];
#pragma unroll
    for (int j = 0; j < NIN; j++) {
        const int idx = t + 256 * j, ci = idx / T::PLANE, r = idx % T::PLANE;
        const int ts = r / (T::TH * T::TW), ry = (r / T::TW) % T::TH, rx = r % T::TW;
        const int gy = y0 - 1 + ry, gx = rx - 1, n = n0 + ts;
        const bool ok = idx < IN_ELEMS && n < N && gy >= 0 && gy < WI && gx >= 0 && gx < WI;
        off_in[j] = ok ? ((n * CI + ci) * WI + gy) * WI + gx : -1;
        ci_in[j] = ci;
    }
#pragma unroll
    for (int j = 0; j < NW4; j++) {
        const int idx = t + 256 * j, q = idx % (COT / 4), rest = idx / (COT / 4), ci = rest % KCT, tap = rest / KCT;
        off_w[j] = (idx < W4_ELEMS && co0 + 4 * q < CO) ? (tap * CI + ci) * CO + co0 + 4 * q : -1;
        ci_w[j] = ci;
    }
    auto issue_chunk = [&](int c0, int stage) {
        float* sb = s_buf + stage * BUF;
        const float* in_c = in + (size_t)c0 * WI * WI;
        const float* w_c = wp + (size_t)c0 * CO;
#pragma unroll
        for (int j = 0; j < NIN; j++) {
            const float* src = (off_in[j] >= 0 && c0 + ci_in[j] < CI) ? in_c + off_in[j] : lgt_zero_pad;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(sb + 256 * j + 64 * wave), 4, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NW4; j++) {
            const float* src = (off_w[j] >= 0 && c0 + ci_w[j] < CI) ? w_c + off_w[j] : lgt_zero_pad;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(sb + IN_PAD + 4 * (256 * j + 64 * wave)),
                                             16, 0, 0);
        }
    };
    issue_chunk(0, 0);
    int stage = 0;
    for (int c0 = 0; c0 < CI; c0 += KCT, stage ^= 1) {
        __syncthreads();   // own loads landed (vmcnt(0)) + every wave is done with the other stage
        if (c0 + KCT < CI) issue_chunk(c0 + KCT, stage ^ 1);
        const float* s_in = s_buf + stage * BUF;
        const float* s_w = s_in + IN_PAD;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int ky = tap / 3, kx = tap % 3;
#pragma unroll
            for (int k0 = 0; k0 < KC; k0 += 2) {
                const int ci = ks * KC + k0 + kh;   // the wave's slice of the staged channels
                float a[CB], b[PB];
#pragma unroll
                for (int j = 0; j < CB; j++) a[j] = s_w[(tap * KCT + ci) * COT + aoff + 32 * j];
#pragma unroll
                for (int i = 0; i < PB; i++) b[i] = s_in[ci * T::PLANE + boff[i] + ky * T::TW + kx];
#pragma unroll
                for (int i = 0; i < PB; i++)
#pragma unroll
                    for (int j = 0; j < CB; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[i], acc[i][j], 0, 0, 0);
            }
        }
    }
    if (KS > 1) {   // the K slices of a tile are added in slice order by the slice-0 wave
        static_assert(KS == 1 || (PB == 1 && CB == 1 && WPX == 1), "K split: one 32 x 32 tile per workgroup");
        __syncthreads();
        if (ks > 0)
#pragma unroll
            for (int r = 0; r < 16; r++) s_buf[(ks - 1) * 1024 + r * 64 + lane] = acc[0][0][r];
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int k = 0; k < KS - 1; k++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[0][0][r] += s_buf[k * 1024 + r * 64 + lane];
    }
    // epilogue: the 16 bias values of a channel block are fetched together (a load + wait per store would cost as much
    // as the K loop of a 64-channel layer); CO is a multiple of 32, so a channel block is inside or outside as a whole
    size_t pix[PB];
    bool okp[PB];
#pragma unroll
    for (int i = 0; i < PB; i++) {
        const int q = (wpx * PB + i) * 32 + lm;
        const int n = n0 + q / (T::TR * WI), y = y0 + (q / WI) % T::TR, x = q % WI;
        okp[i] = n < N;
        pix[i] = (size_t)n * CO * WI * WI + (size_t)y * WI + x;
    }
#pragma unroll
    for (int j = 0; j < CB; j++) {
        const int cob = co0 + (wco * CB + j) * 32;
        if (cob >= CO) continue;
        float bv[16];
#pragma unroll
        for (int r = 0; r < 16; r++) bv[r] = bias ? bias[cob + (r & 3) + 8 * (r >> 2) + 4 * kh] : 0.0f;
#pragma unroll
        for (int i = 0; i < PB; i++) {
            if (!okp[i]) continue;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = cob + (r & 3) + 8 * (r >> 2) + 4 * kh;
                out[pix[i] + (size_t)co * WI * WI] = acc[i][j][r] + bv[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ conv wgrad
// partial[s][tap][ci][co] = sum over the pixel tiles of slice s of a[n][ci][y+ky-1][x+kx-1] * dx[n][co][y][x]
// Workgroup: 32 ci x 64 co, six waves = 2 blocks of 32 output channels x 3 kernel rows; a wave owns the three tap
// accumulators of its row (M = 32 input channels read at the tap's halo offset, N = 32 output channels, K = pixels).
// The input halo tile and the dX tile of kWgTile pixels stream into a double-buffered LDS image with global_load_lds
// (slot idx = t + 384 j lands at float idx; the odd row strides that keep the operand reads conflict-free are slots that
// fetch the zero word); source offsets relative to the tile origin are computed once.  ~100 VGPRs, 62 KB LDS: two
// workgroups = 12 waves per CU, three per SIMD.
constexpr int kWgTile = 64, kWgThreads = 384;
template <int WI>
__global__ __launch_bounds__(kWgThreads, 2) void lgt_wgrad_kernel(const float* __restrict__ a, const float* __restrict__ dx,
                                                                float* __restrict__ partial, int N, int CI, int CO, int ntiles) {
    using T = Tile<WI, kWgTile>;
    constexpr int SD = kWgTile + 1, SI = T::PLANE | 1, NT = kWgThreads;
    constexpr int NSD = (64 * SD + NT - 1) / NT, NSI = (32 * SI + NT - 1) / NT, BUF = (NSD + NSI) * NT;
    __shared__ __attribute__((aligned(16))) float s_buf[2 * BUF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 31, kh = lane >> 5;
    const int wc = wave & 1, ky = wave >> 1;
    const int co0 = blockIdx.y * 64, ci0 = blockIdx.z * 32;
    const bool active = co0 + wc * 32 < CO;

    f32x16 acc[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[k][r] = 0.0f;

    // tile-invariant part of the source offsets (relative to sample n0, row y0) and, packed four to a register, a class byte
    // per slot: bit 0 = never loads (padding slot, channel or column outside), bit 1 = top halo row (outside the image when
    // the tile starts at row 0), bit 2 = bottom halo row (outside when the tile ends at the last row), bits 4-7 = sample
    // within the tile.  Per tile a wave-uniform mask says which classes are dead: two VALU per slot decide the source.
    int rel_d[NSD], rel_i[NSI];
    unsigned cls_i[(NSI + 3) / 4], cls_d[(NSD + 3) / 4];
#pragma unroll
    for (int j = 0; j < (NSI + 3) / 4; j++) cls_i[j] = 0;
#pragma unroll
    for (int j = 0; j < (NSD + 3) / 4; j++) cls_d[j] = 0;
#pragma unroll
    for (int j = 0; j < NSD; j++) {
        const int idx = t + NT * j, co = idx / SD, q = idx % SD;
        const int ts = q / (T::TR * WI), row = (q / WI) % T::TR, x = q % WI;
        const bool ok = idx < 64 * SD && q < kWgTile && co0 + co < CO;
        rel_d[j] = ok ? ((ts * CO + co0 + co) * WI + row) * WI + x : 0;
        cls_d[j >> 2] |= (unsigned)((ok ? 0 : 1) | (ts << 4)) << (8 * (j & 3));
    }
#pragma unroll
    for (int j = 0; j < NSI; j++) {
        const int idx = t + NT * j, ci = idx / SI, r = idx % SI;
        const int ts = r / (T::TH * T::TW), ry = (r / T::TW) % T::TH, rx = r % T::TW;
        const bool ok = idx < 32 * SI && r < T::PLANE && ci0 + ci < CI && rx >= 1 && rx <= WI;
        rel_i[j] = ok ? ((ts * CI + ci0 + ci) * WI + ry - 1) * WI + rx - 1 : 0;
        cls_i[j >> 2] |= (unsigned)((ok ? 0 : 1) | (ry == 0 ? 2 : 0) | (ry == T::TH - 1 ? 4 : 0) | (ts << 4)) << (8 * (j & 3));
    }
    auto issue_tile = [&](int tile, int stage) {
        float* sb = s_buf + stage * BUF;
        const int n0 = (tile / T::BANDS) * T::TS, y0 = (tile % T::BANDS) * T::TR;
        const float* d0 = dx + ((size_t)n0 * CO * WI + y0) * WI;
        const float* a0 = a + ((size_t)n0 * CI * WI + y0) * WI;
        const unsigned dead = 1u | (y0 == 0 ? 2u : 0u) | (y0 + T::TR >= WI ? 4u : 0u);   // wave-uniform
#pragma unroll
        for (int j = 0; j < NSD; j++) {
            bool off = (cls_d[j >> 2] & (1u << (8 * (j & 3)))) != 0;
            if (T::TS > 1) off = off || n0 + (int)((cls_d[j >> 2] >> (8 * (j & 3) + 4)) & 15u) >= N;
            const float* src = off ? lgt_zero_pad : d0 + rel_d[j];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(sb + NT * j + 64 * wave), 4, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NSI; j++) {
            bool off = (cls_i[j >> 2] & (dead << (8 * (j & 3)))) != 0;
            if (T::TS > 1) off = off || n0 + (int)((cls_i[j >> 2] >> (8 * (j & 3) + 4)) & 15u) >= N;
            const float* src = off ? lgt_zero_pad : a0 + rel_i[j];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(sb + NT * (NSD + j) + 64 * wave), 4, 0, 0);
        }
    };
    int stage = 0;
    if ((int)blockIdx.x < ntiles) issue_tile(blockIdx.x, 0);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, stage ^= 1) {
        __syncthreads();   // own loads landed (vmcnt(0)) + every wave is done with the other stage
        if (tile + (int)gridDim.x < ntiles) issue_tile(tile + gridDim.x, stage ^ 1);
        if (active) {
            // pixel q0 + kh sits right of the even pixel q0 in the same image row: halo(q0 + kh) = halo(q0) + kh, so the
            // fully unrolled loop reads at compile-time offsets from two per-lane base pointers (no VALU between MFMAs)
            const float* bb = s_buf + stage * BUF + (wc * 32 + lm) * SD + kh;
            const float* ab = s_buf + stage * BUF + NSD * NT + lm * SI + ky * T::TW + kh;
#pragma unroll
            for (int q0 = 0; q0 < kWgTile; q0 += 2) {
                const float b = bb[q0];
                const float* ai = ab + T::halo(q0);
#pragma unroll
                for (int kx = 0; kx < 3; kx++) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[kx], b, acc[kx], 0, 0, 0);
            }
        }
    }
    if (!active) return;
    const int co = co0 + wc * 32 + lm;
#pragma unroll
    for (int kx = 0; kx < 3; kx++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ci = ci0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (ci < CI && co < CO) partial[(((size_t)blockIdx.x * 9 + ky * 3 + kx) * CI + ci) * CO + co] = acc[kx][r];
        }
}

// gw[co][ci][tap] = sum_s partial[s][tap][ci][co]   (fixed order)
__global__ void lgt_wreduce_kernel(const float* __restrict__ partial, int S, int CI, int CO, float* __restrict__ gw) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n = 9 * CI * CO;
    if (e >= n) return;
    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // four interleaved chains (loads in flight), combined in a fixed order
    int k = 0;
    for (; k + 4 <= S; k += 4)
#pragma unroll
        for (int u = 0; u < 4; u++) s4[u] += partial[(size_t)(k + u) * n + e];
    for (; k < S; k++) s4[0] += partial[(size_t)k * n + e];
    const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    const int co = e % CO, ci = (e / CO) % CI, tap = e / (CO * CI);
    gw[((size_t)co * CI + ci) * 9 + tap] = s;
}

// w[co][ci][tap] -> wpf[tap][ci][co] (forward) and wpd[8-tap][co][ci] (backward-data: taps mirrored, channels swapped);
// all conv layers in one launch
__global__ void lgt_pack_kernel(PackTable T) {
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    int l = 0;
    while (l < T.n && g >= T.end[l]) l++;
    if (l >= T.n) return;
    const int e = (int)(g - (l ? T.end[l - 1] : 0u)), CI = T.ci[l], CO = T.co[l];
    const int tap = e % 9, ci = (e / 9) % CI, co = e / (9 * CI);
    const float v = T.w[l][e];
    T.wpf[l][((size_t)tap * CI + ci) * CO + co] = v;
    T.wpd[l][((size_t)(8 - tap) * CO + co) * CI + ci] = v;
}

constexpr int kMaxSplit = 512;                  // backward-weights pixel slices (partial sums) per layer
constexpr size_t kMaxPartialFloats = 96u << 20; // ... bounded by 384 MiB of partial sums
// pixel slices of a backward-weights launch: enough workgroups (slices x channel blocks) for two per CU, bounded memory
int wgrad_split(int ntiles, size_t nw, int blocks) {
    const size_t cap = std::max<size_t>(8, kMaxPartialFloats / nw);
    const size_t want = std::max<size_t>(8, (size_t)(1024 / std::max(1, blocks)));
    return (int)std::min<size_t>(std::min<size_t>((size_t)ntiles, std::min<size_t>(want, (size_t)kMaxSplit)), cap);
}
int conv_tiles(int wi, int N, int tile) {   // pixel tiles of `tile` pixels covering N samples
    const int hw = wi * wi;
    return hw >= tile ? N * (hw / tile) : (N + tile / hw - 1) / (tile / hw);
}
// grid of a backward-weights launch: x = pixel slices (one partial sum each), y / z = blocks of 64 output / 32 input channels
struct WgradGrid { int ntiles, slices; unsigned cob, cib; };
WgradGrid wgrad_grid(int wi, int N, int CI, int CO) {
    const unsigned cob = lgt_cdiv(CO, 64), cib = lgt_cdiv(CI, 32);
    const int ntiles = conv_tiles(wi, N, kWgTile);
    return {ntiles, wgrad_split(ntiles, (size_t)9 * CI * CO, (int)(cob * cib)), cob, cib};
}

}  // namespace

void lgt_pack(const PackTable& table, hipStream_t s) {
    const unsigned end = table.n ? table.end[table.n - 1] : 0u;
    hipLaunchKernelGGL(lgt_pack_kernel, dim3(lgt_cdiv(end, 256)), dim3(256), 0, s, table);
}

// workgroups of a shape below which the next smaller shape is launched: one workgroup per CU is where the larger tile
// stops paying (swept over batches 16..512: 256 / 256 is the best pair, e.g. batch 256 3.30 ms vs 3.47 with 512 / 256)
// (the thresholds are the caller's: LgtConvCut, LG_TRAIN_CONV_SMALL / LG_TRAIN_CONV_SPLIT for tuning runs)
void lgt_conv(LgtConvCut cut, int wi, const float* in, const float* wp, const float* bias, float* out, int N, int CI, int CO,
              hipStream_t s) {
    const unsigned cb = (unsigned)((CO + 63) / 64), cb32 = (unsigned)((CO + 31) / 32);
    const bool small = conv_tiles(wi, N, 256) * (int)cb < cut.small_below;
    const bool split = conv_tiles(wi, N, 64) * (int)cb < cut.split_below && CI >= 32;
#define LGT_CONV(W)                                                                                                    \
    if (split)                                                                                                         \
        hipLaunchKernelGGL((lgt_conv_kernel<W, 1, 1, 1, 4, 8>), dim3(conv_tiles(W, N, 32), cb32), dim3(256), 0, s, in, wp,  \
                           bias, out, N, CI, CO);                                                                      \
    else if (small)                                                                                                    \
        hipLaunchKernelGGL((lgt_conv_kernel<W, 1, 1, 2, 1, 16>), dim3(conv_tiles(W, N, 64), cb), dim3(256), 0, s, in, wp,   \
                           bias, out, N, CI, CO);                                                                      \
    else                                                                                                               \
        hipLaunchKernelGGL((lgt_conv_kernel<W, 2, 2, 4, 1, 8>), dim3(conv_tiles(W, N, 256), cb), dim3(256), 0, s, in, wp,   \
                           bias, out, N, CI, CO);
    switch (wi) {
        case 32: LGT_CONV(32) break;
        case 16: LGT_CONV(16) break;
        case 8: LGT_CONV(8) break;
        default: LGT_CONV(4) break;
    }
#undef LGT_CONV
}

size_t lgt_wgrad_partial_floats(int wi, int N, int CI, int CO) { return (size_t)wgrad_grid(wi, N, CI, CO).slices * 9 * CI * CO; }
void lgt_wgrad(int wi, const float* a, const float* dx, float* partial, float* gw, int N, int CI, int CO, hipStream_t s) {
    const WgradGrid g = wgrad_grid(wi, N, CI, CO);
    const dim3 grid(g.slices, g.cob, g.cib);
#define LGT_WGRAD(W) \
    hipLaunchKernelGGL(lgt_wgrad_kernel<W>, grid, dim3(kWgThreads), 0, s, a, dx, partial, N, CI, CO, g.ntiles);
    switch (wi) {
        case 32: LGT_WGRAD(32) break;
        case 16: LGT_WGRAD(16) break;
        case 8: LGT_WGRAD(8) break;
        default: LGT_WGRAD(4) break;
    }
#undef LGT_WGRAD
    hipLaunchKernelGGL(lgt_wreduce_kernel, dim3(lgt_cdiv((size_t)9 * CI * CO, 256)), dim3(256), 0, s, partial, g.slices, CI, CO, gw);
}
