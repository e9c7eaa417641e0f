// Label-aware isolation (lg_iso.hip; lg_params.label_aware): the chamfer-3 norm, the isolation of a pixel from the two
// transforms, and the launchers.
#pragma once
#include "lg_internal.h"

// Closed-form norm of the (0.955, 1.3693) chamfer mask: with a zero pixel in the image, the two 3x3 raster passes of
// cv2.distanceTransform give min over the zero pixels q of lg_norm3(|p - q|) (a <= b <= 2a: a diagonal step never loses against
// two straight ones, and never beats one).  The device runs the raster passes themselves (lg_iso_sweep_kernel), whose integers
// are OpenCV's by construction; the norm is the independent statement of their result that the CPU tests hold to the oracle.
__host__ __device__ inline uint32_t lg_norm3(int dx, int dy) {
    const uint32_t a = (uint32_t)(dx > dy ? dx : dy), b = (uint32_t)(dx > dy ? dy : dx);
    return (a - b) * LG_A3 + b * LG_B3;
}
// Words per frame of the label-aware mode's `iso_mf` array (zeroed in front of the bit-row pass): [0], [1] whole-frame maxima
// of the two chamfer-3 transforms (atomicMax), [2] != 0: the frame has a pixel of another leaf, [3] unused
#define LG_ISO_MF 4
// isolation of one pixel of the current leaf from the two transforms (oracle lines 401, 404-408 in order and type: float32
// transforms, max + 1e-6 in float32 as numpy adds a Python float to a float32 scalar, the weighted sum in float32)
__host__ __device__ inline float lg_iso_value(uint32_t dc_fix, uint32_t dw_fix, uint32_t maxc, uint32_t maxw, float w_close,
                                              float w_wide, float ramp) {
#pragma clang fp contract(off)
    const float k = 1.0f / 65536.0f;
    const float sc = ((float)dc_fix * k) / ((float)maxc * k + 1e-6f);
    const float sw = ((float)dw_fix * k) / ((float)maxw * k + 1e-6f);
    return (w_close * sc + w_wide * sw) * ramp;
}

// ---- label-aware isolation (lg_iso.hip), every launch over the frames [0, B) of its pointers
// The two transforms of a batch and where the deferred gather / the plane kernel find them.  A frame with iso_mf[.. + 2] == 0
// (no other leaf) is skipped by every kernel: its plane stays the closed form.
struct LgIsoFields {
    const uint32_t* fields;   // [B][2][H][W] 16.16 transforms of 1 - ic (0) and 1 - iw (1)
    const uint32_t* iso_mf;   // [B][LG_ISO_MF]
};
// the generic-width companion of lg_launch_pack_labels: others' bit rows and flag alone, one wave ballot per word
void lg_launch_pack_others(const int16_t* labels, const int32_t* ids_dev, unsigned long long* others, uint32_t* iso_mf, int B, int H,
                           int W, int WW, hipStream_t s);
// dil[0][b] = dilate(others[b], ellipse 30), dil[1][b] = dilate(others[b], ellipse 40) as bit rows (dil: [2][B][H][WW])
void lg_launch_iso_dilate(const unsigned long long* others, unsigned long long* dil, const uint32_t* iso_mf, int B, int H, int W, int WW,
                          hipStream_t s);
// The 3x3 raster passes of cv2.distanceTransform(1 - dil[f][b], DIST_L2, 3) into fields[b][f], forward then backward (two
// launches), and the whole-frame maxima into iso_mf[b][f].  0: queued, -1: width not supported (W > 8192)
int lg_launch_iso_sweeps(const unsigned long long* dil, uint32_t* fields, uint32_t* iso_mf, int B, int H, int W, int WW, uint32_t init0,
                         hipStream_t s);
// dense planes: isolation[b] on the pixels of the current leaf (bit rows `bits`, bounding boxes `win`) from the fields
void lg_launch_iso_plane(const LgIsoFields& f, const unsigned long long* bits, const LgWin* win, float* iso, int B, int H, int W, int WW,
                         float w_close, float w_wide, float ramp_top, float ramp_step, hipStream_t s);
