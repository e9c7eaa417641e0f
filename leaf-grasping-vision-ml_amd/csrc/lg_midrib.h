// GraspPointSelector.detect_midrib (grasp_point_selector.py:829-922) and the CLAHE it runs on (lg_midrib.hip): geometry,
// the float64 ridge walk shared by the host (lg_midrib_walk) and the device, workspace and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "lg_internal.h"
#include "lg_orient.h"

#define LG_MIDRIB_STEPS 20   // np.linspace(0, 1, 20) along the predicted midrib (:881)

// cv::CLAHE geometry (OpenCV clahe.cpp).  When both H and W divide by the tile counts, tile = (W / tiles_x, H / tiles_y);
// otherwise BOTH dimensions are padded at the end by tiles - size % tiles (BORDER_REFLECT_101), so a dimension that divides
// gains a whole extra `tiles` rows / columns.  The padding feeds the histograms only; interpolation runs on H x W.
struct LgClaheGeom {
    int H, W, tiles_x, tiles_y;
    int tw, th;        // tile size on the (padded) histogram image
    int clip;          // max(int(clip_limit * tile area / 256), 1); 0 = no clipping (clip_limit <= 0)
    float lut_scale;   // 255.0f / tile area
    float inv_tw, inv_th;
};

// host: fills g; returns LG_ERR_INVALID for tiles outside 1..64 or H, W < 2
int lg_clahe_geom(int H, int W, double clip_limit, int tiles_x, int tiles_y, LgClaheGeom* g);

__host__ __device__ inline int lg_reflect101(int p, int n) {   // cv::borderInterpolate(BORDER_REFLECT_101), n >= 2
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// OpenCV's 8-bit BGR2GRAY on channel indices 0, 1, 2 (the visualiser hands in RGB: the weights apply by index)
__host__ __device__ inline int lg_bgr2gray(int c0, int c1, int c2) { return (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14; }

// Per-frame set-up of the walk (:870-879), computed on the host from the five float32 values estimate_leaf_orientation
// reports (widened to double).  status: 0 walk, 1 no contour (angle is None), 2 int(minor / 6) == 0 (cv2.line asserts
// thickness > 0: exception, None).
struct LgMidribGeom {
    int status;
    int c0, c1, dx, dy, ww;
    double perp_x, perp_y;   // (-dy / |d| * ww, dx / |d| * ww)
};

inline int lg_midrib_setup(int found, const float* o, LgMidribGeom* g) {
#pragma clang fp contract(off)
    *g = LgMidribGeom{};
    if (!found) return g->status = 1;
    const double angle = o[0], major = o[1], minor = o[2];
    g->c0 = (int)(double)o[3];
    g->c1 = (int)(double)o[4];
    g->dx = (int)(major / 2 * cos(angle));   // int() truncates toward zero, as C's conversion does
    g->dy = (int)(major / 2 * sin(angle));
    g->ww = (int)(minor / 6);
    if (g->ww <= 0) return g->status = 2;
    // ww >= 1 means minor >= 6, so major >= 6 and dx, dy are not both 0
    const double n = sqrt((double)(g->dx * g->dx + g->dy * g->dy));
    g->perp_x = (double)(-g->dy) / n * (double)g->ww;
    g->perp_y = (double)g->dx / n * (double)g->ww;
    return 0;
}

// np.linspace(a, b, n)[i]: a + i * ((b - a) / (n - 1)) for i < n - 1, exactly b for the last; n == 1 gives [a]
__host__ __device__ inline double lg_linspace(double a, double b, int n, int i) {
#pragma clang fp contract(off)
    if (n == 1) return a;
    if (i == n - 1) return b;
    const double step = (b - a) / (double)(n - 1);
    return (double)i * step + a;
}

// centre-line point of step ti (:882-885); 1 if it lies inside the frame
__host__ __device__ inline int lg_midrib_center(const LgMidribGeom& g, int ti, int H, int W, int* x, int* y) {
#pragma clang fp contract(off)
    const double t = lg_linspace(0.0, 1.0, LG_MIDRIB_STEPS, ti);
    *x = (int)((double)(g.c0 - g.dx) + (double)(2 * g.dx) * t);
    *y = (int)((double)(g.c1 - g.dy) + (double)(2 * g.dy) * t);
    return *x >= 0 && *x < W && *y >= 0 && *y < H;
}

// sample si of the perpendicular through (x, y) (:895-898); 1 if it lies inside the frame
__host__ __device__ inline int lg_midrib_sample(const LgMidribGeom& g, int x, int y, int si, int H, int W, int* sx, int* sy) {
#pragma clang fp contract(off)
    const double s = lg_linspace(-1.0, 1.0, g.ww, si);
    *sx = (int)((double)x + s * g.perp_x);
    *sy = (int)((double)y + s * g.perp_y);
    return *sx >= 0 && *sx < W && *sy >= 0 && *sy < H;
}

// Scratch of lg_clahe / lg_detect_midrib, grown on demand (one per handle)
struct LgMidribWs {
    int* hist = nullptr;  size_t hist_cap = 0;          // [B][tiles][256] int32
    uint8_t* lut = nullptr;                             // [B][tiles][256]
    unsigned long long* bits = nullptr;                 // [B][H][WW] mask bit rows (orientation)
    unsigned long long* bits_host = nullptr;            // pinned copy (host contour analysis)
    size_t bits_cap = 0;
    LgWin* win = nullptr;
    uint32_t* box = nullptr;                            // [B][LG_MF] bounding boxes from the bit-row pass (lg_internal.h; zeroed per call)
    LgFrameParams* fp = nullptr;
    LgMidribGeom* geom = nullptr;  LgMidribGeom* geom_host = nullptr;   // [B]
    int32_t* res = nullptr;  int32_t* res_host = nullptr;               // [B][5]: x0, y0, x1, y1, status
    int capB = 0;
    LgOrientWs* orient = nullptr;   // device contour analysis (null: host analysis of every frame)
};
// hist / lut for B * ntiles tiles; with frames != 0 also the per-frame buffers of lg_detect_midrib for B frames of H x W
int lg_midrib_ensure(LgMidribWs*& w, int B, int H, int W, int ntiles, bool frames, bool device_orient, int orient_cap, std::string* err);
void lg_midrib_free(LgMidribWs*& w);

// kernels (lg_midrib.hip).  C == 0: src is gray [B][H][W]; C == 3 / 4: src is the image [B][H][W][C], gray is computed from it
// and `mask` on the fly.  hist must be zeroed on the stream before lg_launch_clahe_hist.
void lg_launch_clahe_hist(const uint8_t* src, const uint8_t* mask, int C, int B, const LgClaheGeom& g, int* hist, hipStream_t s);
void lg_launch_clahe_lut(const int* hist, uint8_t* lut, int B, const LgClaheGeom& g, hipStream_t s);
void lg_launch_clahe_apply(const uint8_t* src, const uint8_t* lut, int B, const LgClaheGeom& g, uint8_t* dst, hipStream_t s);
void lg_launch_midrib_walk(const uint8_t* image, int C, const uint8_t* mask, const uint8_t* lut, int B, const LgClaheGeom& g,
                           const LgMidribGeom* geom, int32_t* res, hipStream_t s);
