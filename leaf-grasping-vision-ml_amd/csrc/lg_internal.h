// Internal declarations that every translation unit of liblgrasp.so (gfx950 only) shares: chamfer and maxfix constants, the tile
// of the plane kernel, LgWin, LgFrameParams, LgSeSpans.  What belongs to one stage is in that stage's header, next to the
// code that runs it; this file ends by including those (all compile as host C++ too), so an includer sees every name.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/leafgrasp.h"

// ---- chamfer constants: 16.16 fixed point of OpenCV's DIST_L2 masks ("Distance transform")
#define LG_A5 65536u        // 1.0
#define LG_B5 91750u        // 1.4
#define LG_C5 143976u       // 2.1969
#define LG_A3 62587u        // 0.955
#define LG_B3 89738u        // 1.3693
#define LG_INIT0 0x1FFFFFFFu  // INT_MAX >> 2 : OpenCV's border initialiser, the default of lg_params.chamfer_init_dist0
#define LG_INF 0x3FFFFFFFu    // "no path yet" inside the DT sweeps (never wins against a real distance)
#define LG_NOSRC 0x20000000u  // 8192 px: with chamfer_init_dist0 up to here OpenCV's border cells hide every distance near LG_INF (make_plan)
#define LG_HCAP 16383u        // run distance of a row without any zero pixel in the image (row search; W <= 8192)
// Words per frame of the `maxfix` array, zeroed by one memset in front of the bit-row pass:
//   [0], [1]  max fixed-point d_in / d_out (atomicMax of the distance transform)
//   [2 .. 6]  the mask's bounding box and area as the bit-row pass accumulates them (LG_BOX_*): every word is a maximum or a
//             sum over the set bits, so all start from 0 -- the two minima are held as W - 1 - x0 and H - 1 - y0; a frame
//             whose area stayed 0 has no set bit, whatever the other four say
#define LG_MF 8
#define LG_BOX_X0 2   // max of W - 1 - x
#define LG_BOX_X1 3   // max of x
#define LG_BOX_Y0 4   // max of H - 1 - y
#define LG_BOX_Y1 5   // max of y
#define LG_BOX_AREA 6 // number of set bits

// ---- final-kernel tile
#define LG_TW 64
#ifndef LG_TH
#define LG_TH 16   // measured at 1080p B=128: 16 -> 1.78 ms (0.69 of HBM peak), 32 -> 1.86 ms, 64 -> 2.11 ms (round 1); round 2, whole library
                   // built with -DLG_TH=32: planes 2.60-2.71 vs 2.66-2.74 ms per 256 frames, top-k 0.33 vs 0.27 ms, dense launch the same
#endif

// Window of the distance-transform sweeps (per frame, written by lg_window_kernel).  The binary leaf mask covers a few
// per cent of a frame, so the sweeps run on the tile-aligned window around its bounding box only:
//   d_in  (distance to the nearest zero pixel): every pixel outside the window is itself a zero pixel -> exactly 0, and
//         enters the window as a 0-valued halo: the windowed two-pass recurrence is the full-frame one, bit for bit.
//   d_out (distance to the leaf; only max d_out is consumed): the two-pass 5x5 chamfer transform equals
//         min over sources of the chamfer NORM (weights satisfy 2a <= c <= a+b, 3b <= 2c), shortest paths stay inside the
//         bounding rectangle of their end points, so the window computed as a stand-alone image is exact inside; outside
//         the window the distance grows monotonically towards the frame border, where lg_dout_border_kernel evaluates
//         the norm in closed form against the leaf's row / column profiles.
// Columns [wx0, wx0 + nw * 64 * E) (clipped to W), rows [wy0, wy1): wx0 % 64 == 0, wy0 % LG_TH == 0, so every tile of
// the fused score-plane kernel is either inside (reads distance_map) or outside (writes zeros to it).
struct LgWin {
    int wx0, nw, wy0, wy1;   // window: first column, active waves (64*E columns each), row range
    int bx0, bx1, by0, by1;  // bounding box of the mask (bx1 < bx0: empty mask -> window = whole frame)
    int skip_out;            // 1: max d_out cannot lie inside the window (see lg_win_from_box): the d_out sweeps of this frame are skipped
    int search_in;           // 1: d_in of this frame comes from the row search (lg_hrun_kernel + lg_dtsearch_kernel), its d_in sweeps are skipped
    int area;                // set bits of the mask
    int pad_[1];
};

struct LgFrameParams {  // per frame: leaf orientation, written by lg_orient_kernel (or by the host analysis for frames it hands back)
    float sin_t, cos_t;
    int has_angle;
    float theta;
};

struct LgSeSpans {  // run-length form of an elliptical structuring element (one span per SE row)
    int n;          // rows
    int anchor;     // k/2
    signed char lo[64];  // first set column - anchor (inclusive); lo > hi => empty row
    signed char hi[64];  // last set column - anchor (inclusive)
};

// ---- the stage headers
#include "lg_bits.h"
#include "lg_contour.h"
#include "lg_dt.h"
#include "lg_finish.h"
#include "lg_iso.h"
#include "lg_patches.h"
#include "lg_planes.h"
#include "lg_topk.h"
