// Score planes (lg_planes.hip): the Gaussian taps of lg_smooth_depth, the near tiles of a frame, the arguments of the fused
// plane kernel, and the launchers.
#pragma once
#include "lg_internal.h"

#define LG_MAX_GAUSS 15   // largest smoothing kernel lg_smooth_depth takes (the fused plane kernel: 1, 3, 5, 7)
struct LgGaussTaps { float k[LG_MAX_GAUSS]; };   // 1-D factor of ImageProcessor's Gaussian (by value in the kernel arguments)

// Near tiles of a frame: the tiles of the fused score-plane kernel (LG_TW x LG_TH, stencil reach `halo` = Gaussian radius + 1)
// whose bit-row test can meet the mask's bounding box [bx0, bx1] x [by0, by1].  The test reads columns tx0-8 .. tx0+LG_TW+7 and
// rows ty0-halo .. ty0+LG_TH-1+halo reflected at the frame border -- at the bottom that reaches up to LG_TH+halo rows above ty0
// (a last tile row of one pixel), at the top it stays inside the tile -- so tile (tx, ty), tx0 = tx * LG_TW, ty0 = ty * LG_TH, is
// near when
//     bx1 >= bx0  &&  bx0 <= tx0 + LG_TW + 7  &&  bx1 >= tx0 - 8  &&  by0 <= ty0 + LG_TH - 1 + halo  &&  by1 >= ty0 - LG_TH - halo.
// Each inequality bounds tx or ty alone: the near tiles are the rectangle [*tx_lo, *tx_hi] x [*ty_lo, *ty_hi] of the frame's
// tile grid.  Returns their number; 0 (an empty box, or one that no tile of the grid reaches) with the rectangle (0, -1, 0, -1).
// Every other tile is constant whatever the mask: key and state byte depend on the tile index alone.  lg_final_kernel, the
// enumeration (lg_near_tiles_kernel) and the host export lg_near_tile_rect run this code.
__host__ __device__ inline int lg_near_tiles(int bx0, int bx1, int by0, int by1, int H, int W, int halo, int* tx_lo, int* tx_hi,
                                             int* ty_lo, int* ty_hi) {
    const int tiles_x = (W + LG_TW - 1) / LG_TW, tiles_y = (H + LG_TH - 1) / LG_TH;
    const int xa = bx0 - (LG_TW + 7), xb = bx1 + 8;                     // xa <= tx0 <= xb
    const int ya = by0 - (LG_TH - 1 + halo), yb = by1 + LG_TH + halo;   // ya <= ty0 <= yb
    const int x_lo = xa > 0 ? (xa + LG_TW - 1) / LG_TW : 0, y_lo = ya > 0 ? (ya + LG_TH - 1) / LG_TH : 0;
    const int x_hi = xb < 0 ? -1 : (xb / LG_TW < tiles_x ? xb / LG_TW : tiles_x - 1);
    const int y_hi = yb < 0 ? -1 : (yb / LG_TH < tiles_y ? yb / LG_TH : tiles_y - 1);
    if (bx1 < bx0 || x_lo > x_hi || y_lo > y_hi) {
        *tx_lo = 0; *tx_hi = -1; *ty_lo = 0; *ty_hi = -1;
        return 0;
    }
    *tx_lo = x_lo; *tx_hi = x_hi; *ty_lo = y_lo; *ty_hi = y_hi;
    return (x_hi - x_lo + 1) * (y_hi - y_lo + 1);
}
__host__ __device__ inline int lg_near_tiles(const LgWin& w, int H, int W, int halo, int* tx_lo, int* tx_hi, int* ty_lo, int* ty_hi) {
    return lg_near_tiles(w.bx0, w.bx1, w.by0, w.by1, H, W, halo, tx_lo, tx_hi, ty_lo, ty_hi);
}

struct LgFinalArgs {
    const float* depth;
    const unsigned long long* bits;
    const unsigned long long* stem_bits;
    const uint32_t* maxfix;       // [B][2] max fixed-point d_in / d_out
    const LgWin* win;             // [B] sweep windows
    int win_wc;                   // columns per sweep wave (64 * E)
    const LgFrameParams* fp;      // [B]
    float* maps[LG_NUM_MAPS];     // [B][H][W] each (may be null except DISTANCE/TRADITIONAL)
    uint8_t* valid;               // [B][H][W] or null
    unsigned long long* tilekeys; // [B][tiles]
    uint8_t* tile_state;          // [B][tiles] or null: 1 = the tile's planes and validity were written, 0 = constant tile
    int sparse;                   // 1: constant tiles write no plane and no validity byte (only their key and state byte)
    int score_only;               // 1 (deferred planes; with sparse): stencil tiles store traditional, validity, flatness and
                                  //   distance = 0 outside the sweep window only; lg_launch_gather computes the other five planes at its windows
    int B, H, W, WW, tiles_x, tiles_y;
    int cxi, cyi;      // floor of the optical centre; (x - cxi) is exact, the fraction is subtracted afterwards
    float cxf, cyf, f;  // fractions in [0,1) and the focal length
    float w_approach, w_sdf, w_flat, w_access;
    float sdf_w_interior, sdf_w_align, sdf_w_sdf, optimal_distance;
    float access_w_dist, access_w_dir, flat_scale;
    float iso_w_close, iso_w_wide, iso_ramp_top, iso_ramp_bottom, iso_inv_max;
    float min_edge_distance, stem_valid_thresh;
    float inv_maxd;
    uint32_t init0;    // lg_params.chamfer_init_dist0
    float inv_2s2, iso_ramp_step;   // 1 / (2 optimal_distance^2) (float32 reciprocal), (ramp_bottom - ramp_top) / (H - 1)
    float k1[7];  // separable 1-D Gaussian: 2 * gauss_r + 1 taps, sigma = size / 6 (image_processor.py:25-32)
    int gauss_r;    // radius of that Gaussian: 0..3 (lg_params.gaussian_size 1, 3, 5, 7)
    int no_skip;    // bit 0: tile-level constant path off, bit 1: wave-level off-leaf shortcut off (LG_NO_SKIP; same results, A/B timing)
    int nt_stores;  // always 0: plain plane stores (1: non-temporal, measured slower; no switch selects it any more, the kernel's text
                    // stays as measured: profiles/NOTES_options.md, section 3)
    int persist;    // from the caller, LgOptions::final_persist: resident workgroups per CU that walk the tiles (< 0: the mode's default)
    int tpw;        // > 0: consecutive tiles per workgroup (from the caller LgOptions::final_tpw; lg_launch_final leaves what the kernel reads)
    // near launch (sparse mode): the workgroups take the entries of the batch's list of near tiles (lg_near_tiles) instead of
    // every tile; the far tiles' keys and state bytes were written by lg_launch_near_tiles.  null: every tile
    const int32_t* near_off;   // [B + 1] DEVICE: first list entry of every frame, near_off[B] = near_total
    int near_total;            // entries of the list this launch takes (the whole batch: the host's copy of near_off[B])
    int near_base;             // list entry of near_off[0] (a launch over the frames [f0, f1) of a batch passes near_off + f0, B = f1 - f0,
                               //   near_base = near_off[f0] and near_total = near_off[f1] - near_off[f0]; the whole batch: 0)
    int near_tpw;              // consecutive list entries per workgroup (>= 1)
};

void lg_launch_final(const LgFinalArgs& a, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// Near tiles of a batch, in front of the near launch of lg_final_kernel (LgFinalArgs::near_off): near_off[b] = near tiles of the
// frames before b (exclusive scan of lg_near_tiles over win[0 .. B), near_off[B] = their total), and every FAR tile's constant
// key and state byte 0 into tilekeys / tile_state -- exactly what lg_final_kernel's constant path stores.  No atomics: the
// same output on every run.  halo: Gaussian radius + 1 of the plane kernel that follows.  near_off_host_dev (or null): the
// device alias of the host's pinned copy of near_off, which the kernel then writes as well.
void lg_launch_near_tiles(const LgWin* win, int B, int H, int W, int halo, int32_t* near_off, int32_t* near_off_host_dev,
                          unsigned long long* tilekeys, uint8_t* tile_state, hipStream_t s);
void lg_launch_smooth(const float* src, float* dst, int B, int H, int W, int S, const LgGaussTaps& taps, hipStream_t s);
