// GraspPointSelector.detect_midrib (scripts/utils/grasp_point_selector.py:829-922) on gfx950:
//   cv2.createCLAHE(clipLimit, tileGridSize).apply (OpenCV clahe.cpp) as three kernels -- per-tile histograms, clip +
//   redistribute + scan into one LUT per tile, bilinear LUT interpolation -- and the ridge walk of :880-907, one workgroup
//   per frame, that evaluates the enhanced image only at the pixels it samples.
// Only what affects the result is computed: the green-channel Otsu threshold, Sobel, Canny and ridge_mask of the reference
// feed nothing.
// The walk's float64 arithmetic and the interpolation's float32 arithmetic must round like numpy / OpenCV: no contraction
// into FMAs anywhere in this file.
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>
#include <string>

#include "lg_midrib.h"

namespace {

constexpr int HT = 256;   // threads per workgroup of every kernel here

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// byte j of a little-endian word array
__device__ inline int byte_at(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255; }

// gray of the masked image at pixel p (mask already known to be set)
__device__ inline int gray_at(const uint8_t* __restrict__ img, int C, size_t p) {
    const uint8_t* q = img + p * C;
    return lg_bgr2gray(q[0], q[1], q[2]);
}

// ---------------------------------------------------------------------------------------------------------------- kernel 1
// grid (tiles * nsplit, B): workgroup = rows [r0, r1) of one tile (padded coordinates) x its tw columns.  Items are 16-pixel
// chunks at x = 16 c, so a wave reads whole 16-byte slots of consecutive rows (uint4; Guideline 13).  Pixels whose gray is
// 0 -- every pixel off the leaf -- are counted in a register and reach bin 0 once per wave; only the others go through the
// LDS histogram.  The image is read only in chunks where the mask has a set byte.
template <int C>
__global__ __launch_bounds__(HT) void lg_clahe_hist_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask,
                                                           LgClaheGeom g, int nsplit, int* __restrict__ hist) {
    __shared__ int sh[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int split = blockIdx.x % nsplit, tile = blockIdx.x / nsplit;
    const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
    const int r0 = tyi * g.th + (split * g.th) / nsplit, r1 = tyi * g.th + ((split + 1) * g.th) / nsplit;
    const int xs = txi * g.tw, xe = xs + g.tw;
    const int c_lo = xs >> 4, cpr = ((xe + 15) >> 4) - c_lo;
    sh[tid] = 0;
    __syncthreads();
    const int H = g.H, W = g.W;
    const uint8_t* lead = C == 0 ? src : mask;   // the bytes that decide bin 0: gray itself, or the mask
    int zeros = 0;
    const int items = (r1 - r0) * cpr;
    for (int i = tid; i < items; i += HT) {
        const int r = i / cpr;
        const int x0 = (c_lo + i - r * cpr) << 4;
        const int y = lg_reflect101(r0 + r, H);
        const size_t row = ((size_t)b * H + y) * W;
        const uint8_t* lp = lead + row + x0;
        const bool fast = x0 >= xs && x0 + 16 <= xe && x0 + 16 <= W && (((uintptr_t)lp) & 15) == 0;
        if (fast) {
            const uint4 mv = *reinterpret_cast<const uint4*>(lp);
            const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
            if constexpr (C == 0) {
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int v = byte_at(m, k);
                    if (v) atomicAdd(&sh[v], 1); else zeros++;
                }
            } else {
                if ((m[0] | m[1] | m[2] | m[3]) == 0) {
                    zeros += 16;
                } else {
                    const uint8_t* ip = src + (row + x0) * C;
                    if ((((uintptr_t)ip) & 15) == 0) {
                        uint32_t px[4 * C];
#pragma unroll
                        for (int q = 0; q < C; q++) {
                            const uint4 v = reinterpret_cast<const uint4*>(ip)[q];
                            px[4 * q] = v.x; px[4 * q + 1] = v.y; px[4 * q + 2] = v.z; px[4 * q + 3] = v.w;
                        }
#pragma unroll
                        for (int k = 0; k < 16; k++) {
                            const int v = byte_at(m, k) ? lg_bgr2gray(byte_at(px, C * k), byte_at(px, C * k + 1), byte_at(px, C * k + 2)) : 0;
                            if (v) atomicAdd(&sh[v], 1); else zeros++;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 16; k++) {
                            const int v = byte_at(m, k) ? gray_at(src, C, row + x0 + k) : 0;
                            if (v) atomicAdd(&sh[v], 1); else zeros++;
                        }
                    }
                }
            }
        } else {   // tile edge inside the chunk, reflected padding, or an unaligned row: pixel by pixel
            for (int k = 0; k < 16; k++) {
                const int xp = x0 + k;
                if (xp < xs || xp >= xe) continue;
                const size_t p = row + lg_reflect101(xp, W);
                int v;
                if (C == 0) v = src[p];
                else v = mask[p] ? gray_at(src, C, p) : 0;
                if (v) atomicAdd(&sh[v], 1); else zeros++;
            }
        }
    }
    zeros = wave_sum(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&sh[0], zeros);
    __syncthreads();
    const int ntiles = g.tiles_x * g.tiles_y;
    if (sh[tid]) atomicAdd(&hist[((size_t)b * ntiles + tile) * 256 + tid], sh[tid]);
}

// ---------------------------------------------------------------------------------------------------------------- kernel 2
// grid (tiles, B), one lane per bin: clip, redistribute (batch to every bin, the residual one count at a time at bins 0, step,
// 2 step, ...), inclusive scan, lut = saturate_cast<uchar>(float(cumsum) * lut_scale) (round half to even)
__global__ __launch_bounds__(HT) void lg_clahe_lut_kernel(const int* __restrict__ hist, uint8_t* __restrict__ lut, LgClaheGeom g) {
    __shared__ int sh[256];
    __shared__ int clipped;
    const int i = threadIdx.x;
    const size_t idx = ((size_t)blockIdx.y * (g.tiles_x * g.tiles_y) + blockIdx.x) * 256 + i;
    int h = hist[idx];
    if (g.clip > 0) {
        if (i == 0) clipped = 0;
        __syncthreads();
        const int ex = wave_sum(h > g.clip ? h - g.clip : 0);
        if ((i & 63) == 0 && ex) atomicAdd(&clipped, ex);
        __syncthreads();
        const int c = clipped;
        h = min(h, g.clip);
        const int batch = c / 256, residual = c - batch * 256;
        h += batch;
        if (residual) {
            const int step = max(256 / residual, 1);
            if (i % step == 0 && i / step < residual) h++;
        }
    }
    sh[i] = h;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {
        const int v = i >= off ? sh[i - off] : 0;
        __syncthreads();
        sh[i] += v;
        __syncthreads();
    }
    const int r = __float2int_rn((float)sh[i] * g.lut_scale);
    lut[idx] = (uint8_t)min(max(r, 0), 255);
}

// CLAHE_Interpolation_Body: value of gray v at (x, y) from the four surrounding tiles' LUTs (float32, round half to even)
__device__ inline int clahe_value(const uint8_t* __restrict__ lut, const LgClaheGeom& g, int x, int y, int v) {
    const float txf = (float)x * g.inv_tw - 0.5f;
    int tx1 = (int)floorf(txf);
    int tx2 = tx1 + 1;
    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
    tx1 = min(max(tx1, 0), g.tiles_x - 1);
    tx2 = min(tx2, g.tiles_x - 1);
    const float tyf = (float)y * g.inv_th - 0.5f;
    int ty1 = (int)floorf(tyf);
    int ty2 = ty1 + 1;
    const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
    ty1 = min(max(ty1, 0), g.tiles_y - 1);
    ty2 = min(ty2, g.tiles_y - 1);
    const uint8_t* l1 = lut + (size_t)ty1 * g.tiles_x * 256;
    const uint8_t* l2 = lut + (size_t)ty2 * g.tiles_x * 256;
    const float res = ((float)l1[tx1 * 256 + v] * xa1 + (float)l1[tx2 * 256 + v] * xa) * ya1 +
                      ((float)l2[tx1 * 256 + v] * xa1 + (float)l2[tx2 * 256 + v] * xa) * ya;
    return min(max(__float2int_rn(res), 0), 255);
}

// ---------------------------------------------------------------------------------------------------------------- kernel 3
// lg_clahe's output: one 16-pixel chunk of a row per item (uint4 in / out where the row is aligned)
__global__ __launch_bounds__(HT) void lg_clahe_apply_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ lut,
                                                            LgClaheGeom g, long long items, uint8_t* __restrict__ dst) {
    const int cpr = (g.W + 15) >> 4;
    const size_t lut_frame = (size_t)g.tiles_x * g.tiles_y * 256;
    for (long long it = (long long)blockIdx.x * HT + threadIdx.x; it < items; it += (long long)gridDim.x * HT) {
        const long long row = it / cpr;
        const int x0 = (int)(it - row * cpr) << 4;
        const int b = (int)(row / g.H), y = (int)(row - (long long)b * g.H);
        const uint8_t* fl = lut + (size_t)b * lut_frame;
        const size_t p = (size_t)row * g.W + x0;
        if (x0 + 16 <= g.W && (((uintptr_t)(src + p) | (uintptr_t)(dst + p)) & 15) == 0) {
            const uint4 sv = *reinterpret_cast<const uint4*>(src + p);
            const uint32_t s4[4] = {sv.x, sv.y, sv.z, sv.w};
            uint32_t d4[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; k++) d4[k >> 2] |= (uint32_t)clahe_value(fl, g, x0 + k, y, byte_at(s4, k)) << (8 * (k & 3));
            *reinterpret_cast<uint4*>(dst + p) = make_uint4(d4[0], d4[1], d4[2], d4[3]);
        } else {
            for (int k = 0; k < 16 && x0 + k < g.W; k++) dst[p + k] = (uint8_t)clahe_value(fl, g, x0 + k, y, src[p + k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- kernel 4
// One workgroup per frame: the 20 x ww samples of :880-904 spread over the lanes.  A sample counts where it lies in the
// frame and on the mask; its enhanced value is CLAHE of the masked gray there.  Per step the FIRST maximum wins (np.argmax):
// key = (value + 1) << 22 | (2^22 - 1 - sample index), atomicMax in LDS.  ww = int(minor / 6) < 2^22 for any frame the
// orientation accepts (minor <= the frame diagonal).
__global__ __launch_bounds__(HT) void lg_midrib_walk_kernel(const uint8_t* __restrict__ img, int C, const uint8_t* __restrict__ mask,
                                                            const uint8_t* __restrict__ lut, LgClaheGeom g,
                                                            const LgMidribGeom* __restrict__ geoms, int32_t* __restrict__ res) {
    __shared__ int key[LG_MIDRIB_STEPS];
    const int b = blockIdx.x, tid = threadIdx.x, H = g.H, W = g.W;
    const LgMidribGeom gm = geoms[b];
    int32_t* r = res + 5 * (size_t)b;
    if (gm.status) {
        if (tid == 0) { r[0] = r[1] = r[2] = r[3] = -1; r[4] = gm.status; }
        return;
    }
    if (tid < LG_MIDRIB_STEPS) key[tid] = 0;
    __syncthreads();
    const size_t fpx = (size_t)b * H * W;
    const uint8_t* fl = lut + (size_t)b * g.tiles_x * g.tiles_y * 256;
    const int n = LG_MIDRIB_STEPS * gm.ww;
    for (int i = tid; i < n; i += HT) {
        const int ti = i / gm.ww, si = i - ti * gm.ww;
        int x, y, sx, sy;
        if (!lg_midrib_center(gm, ti, H, W, &x, &y)) continue;
        if (!lg_midrib_sample(gm, x, y, si, H, W, &sx, &sy)) continue;
        const size_t p = fpx + (size_t)sy * W + sx;
        if (!mask[p]) continue;
        const int v = clahe_value(fl, g, sx, sy, gray_at(img, C, p));
        atomicMax(&key[ti], ((v + 1) << 22) | ((1 << 22) - 1 - si));
    }
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int ti = 0; ti < LG_MIDRIB_STEPS; ti++) {
            if (!key[ti]) continue;
            const int si = (1 << 22) - 1 - (key[ti] & ((1 << 22) - 1));
            int x, y, sx, sy;
            lg_midrib_center(gm, ti, H, W, &x, &y);
            lg_midrib_sample(gm, x, y, si, H, W, &sx, &sy);
            if (cnt == 0) { r[0] = sx; r[1] = sy; }
            r[2] = sx; r[3] = sy;
            cnt++;
        }
        if (cnt < 2) r[0] = r[1] = r[2] = r[3] = -1;
        r[4] = cnt < 2 ? 3 : 0;
    }
}

template <typename T>
hipError_t dalloc(T** p, size_t n) { return hipMalloc((void**)p, n * sizeof(T)); }

}  // namespace

int lg_clahe_geom(int H, int W, double clip_limit, int tiles_x, int tiles_y, LgClaheGeom* g) {
    if (H < 2 || W < 2 || tiles_x < 1 || tiles_x > 64 || tiles_y < 1 || tiles_y > 64 || !(clip_limit == clip_limit))
        return LG_ERR_INVALID;
    g->H = H; g->W = W; g->tiles_x = tiles_x; g->tiles_y = tiles_y;
    if (W % tiles_x == 0 && H % tiles_y == 0) {
        g->tw = W / tiles_x; g->th = H / tiles_y;
    } else {
        g->tw = (W + tiles_x - W % tiles_x) / tiles_x;
        g->th = (H + tiles_y - H % tiles_y) / tiles_y;
    }
    const int area = g->tw * g->th;
    g->clip = 0;
    if (clip_limit > 0.0) {
        const double c = clip_limit * area / 256;
        g->clip = c >= 2147483647.0 ? 2147483647 : std::max((int)c, 1);
    }
    g->lut_scale = 255.0f / (float)area;
    g->inv_tw = 1.0f / (float)g->tw;
    g->inv_th = 1.0f / (float)g->th;
    return LG_OK;
}

void lg_midrib_free(LgMidribWs*& w) {
    if (!w) return;
    auto F = [](void* p) { if (p) hipFree(p); };
    auto HF = [](void* p) { if (p) hipHostFree(p); };
    F(w->hist); F(w->lut); F(w->bits); F(w->win); F(w->box); F(w->fp); F(w->geom); F(w->res);
    HF(w->bits_host); HF(w->geom_host); HF(w->res_host);
    lg_orient_free(w->orient);
    delete w;
    w = nullptr;
}

int lg_midrib_ensure(LgMidribWs*& w, int B, int H, int W, int ntiles, bool frames, bool device_orient, int orient_cap, std::string* err) {
    if (!w) w = new LgMidribWs();
    hipError_t rc = hipSuccess;
    auto A = [&](hipError_t r) { if (rc == hipSuccess) rc = r; };
    const size_t nh = (size_t)B * ntiles * 256;
    if (nh > w->hist_cap) {
        hipDeviceSynchronize();
        if (w->hist) hipFree(w->hist);
        if (w->lut) hipFree(w->lut);
        w->hist = nullptr; w->lut = nullptr; w->hist_cap = 0;
        A(dalloc(&w->hist, nh)); A(dalloc(&w->lut, nh));
        if (rc != hipSuccess) { if (err) *err = std::string("midrib histograms: ") + hipGetErrorString(rc); return LG_ERR_NOMEM; }
        w->hist_cap = nh;
    }
    if (!frames) return LG_OK;
    const size_t nbits = (size_t)B * H * ((W + 63) / 64);
    if (nbits > w->bits_cap) {
        hipDeviceSynchronize();
        if (w->bits) hipFree(w->bits);
        if (w->bits_host) hipHostFree(w->bits_host);
        w->bits = w->bits_host = nullptr; w->bits_cap = 0;
        A(dalloc(&w->bits, nbits)); A(hipHostMalloc((void**)&w->bits_host, nbits * sizeof(unsigned long long)));
        if (rc != hipSuccess) { if (err) *err = std::string("midrib bit rows: ") + hipGetErrorString(rc); return LG_ERR_NOMEM; }
        w->bits_cap = nbits;
    }
    if (B > w->capB) {
        hipDeviceSynchronize();
        auto F = [](void* p) { if (p) hipFree(p); };
        auto HF = [](void* p) { if (p) hipHostFree(p); };
        F(w->win); F(w->box); F(w->fp); F(w->geom); F(w->res); HF(w->geom_host); HF(w->res_host);
        w->win = nullptr; w->box = nullptr; w->fp = nullptr; w->geom = w->geom_host = nullptr; w->res = w->res_host = nullptr; w->capB = 0;
        A(dalloc(&w->win, B)); A(dalloc(&w->box, (size_t)B * LG_MF)); A(dalloc(&w->fp, B)); A(dalloc(&w->geom, B)); A(dalloc(&w->res, (size_t)B * 5));
        A(hipHostMalloc((void**)&w->geom_host, sizeof(LgMidribGeom) * B));
        A(hipHostMalloc((void**)&w->res_host, sizeof(int32_t) * 5 * B));
        if (rc != hipSuccess) { if (err) *err = std::string("midrib frame buffers: ") + hipGetErrorString(rc); return LG_ERR_NOMEM; }
        w->capB = B;
    }
    if (device_orient) {
        // no device scratch: the host contour analysis of every frame gives the same values (lg_leaf_orientation's hand-off)
        if (lg_orient_ensure(w->orient, B, H, orient_cap, nullptr)) {
            lg_orient_free(w->orient);
            (void)hipGetLastError();
        }
    } else {
        lg_orient_free(w->orient);
    }
    return LG_OK;
}

void lg_launch_clahe_hist(const uint8_t* src, const uint8_t* mask, int C, int B, const LgClaheGeom& g, int* hist, hipStream_t s) {
    const int ntiles = g.tiles_x * g.tiles_y;
    // enough workgroups for the part at small B: split a tile's rows until there are ~2048 of them
    const int nsplit = std::max(1, std::min(g.th, (2048 + ntiles * B - 1) / (ntiles * B)));
    const dim3 grid(ntiles * nsplit, B);
    if (C == 0) hipLaunchKernelGGL(lg_clahe_hist_kernel<0>, grid, dim3(HT), 0, s, src, mask, g, nsplit, hist);
    else if (C == 3) hipLaunchKernelGGL(lg_clahe_hist_kernel<3>, grid, dim3(HT), 0, s, src, mask, g, nsplit, hist);
    else hipLaunchKernelGGL(lg_clahe_hist_kernel<4>, grid, dim3(HT), 0, s, src, mask, g, nsplit, hist);
}

void lg_launch_clahe_lut(const int* hist, uint8_t* lut, int B, const LgClaheGeom& g, hipStream_t s) {
    hipLaunchKernelGGL(lg_clahe_lut_kernel, dim3(g.tiles_x * g.tiles_y, B), dim3(HT), 0, s, hist, lut, g);
}

void lg_launch_clahe_apply(const uint8_t* src, const uint8_t* lut, int B, const LgClaheGeom& g, uint8_t* dst, hipStream_t s) {
    const long long items = (long long)B * g.H * ((g.W + 15) >> 4);
    const long long blocks = std::min<long long>((items + HT - 1) / HT, 16384);
    hipLaunchKernelGGL(lg_clahe_apply_kernel, dim3((unsigned)blocks), dim3(HT), 0, s, src, lut, g, items, dst);
}

void lg_launch_midrib_walk(const uint8_t* image, int C, const uint8_t* mask, const uint8_t* lut, int B, const LgClaheGeom& g,
                           const LgMidribGeom* geom, int32_t* res, hipStream_t s) {
    hipLaunchKernelGGL(lg_midrib_walk_kernel, dim3(B), dim3(HT), 0, s, image, C, mask, lut, g, geom, res);
}

// The walk on the host over a given enhanced image: the same set-up, centre-line and sample arithmetic as the kernel.
int lg_midrib_walk(const uint8_t* enhanced, const uint8_t* mask, int H, int W, int found, const float* orient, int32_t* out,
                   int32_t* status) {
    if (!enhanced || !mask || !out || !status || H < 1 || W < 1 || (found && !orient)) return LG_ERR_INVALID;
    LgMidribGeom g;
    out[0] = out[1] = out[2] = out[3] = -1;
    if ((*status = lg_midrib_setup(found, orient, &g))) return LG_OK;
    int cnt = 0;
    for (int ti = 0; ti < LG_MIDRIB_STEPS; ti++) {
        int x, y;
        if (!lg_midrib_center(g, ti, H, W, &x, &y)) continue;
        int best = -1, bx = 0, by = 0;
        for (int si = 0; si < g.ww; si++) {
            int sx, sy;
            if (!lg_midrib_sample(g, x, y, si, H, W, &sx, &sy)) continue;
            const size_t p = (size_t)sy * W + sx;
            if (mask[p] && enhanced[p] > best) { best = enhanced[p]; bx = sx; by = sy; }
        }
        if (best < 0) continue;
        if (cnt == 0) { out[0] = bx; out[1] = by; }
        out[2] = bx; out[3] = by;
        cnt++;
    }
    if (cnt < 2) out[0] = out[1] = out[2] = out[3] = -1;
    *status = cnt < 2 ? 3 : 0;
    return LG_OK;
}
