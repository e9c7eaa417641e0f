// Distance transform (lg_dt.hip): launchers of its kernels and the choice between the forms of the sweep-free row search.
#pragma once
#include "lg_internal.h"

// columns per sweep wave / waves per sweep workgroup for width W (0 if unsupported)
int lg_dt_geometry(int W, int* waves);
// search_mode: 0 = d_in by the two sweeps for every frame, 1 = by the row search wherever it applies (a non-empty mask with
// at least one zero pixel), 2 = the row search when the batch's estimated search work stays below the sweeps' latency
// mf: what lg_launch_pack_bits / lg_launch_pack_labels accumulated on the same stream
// init0: lg_params.chamfer_init_dist0 of a call whose windows the distance transforms will use (lg_dt_far); the orientation-only
// callers leave it out
void lg_launch_window(const uint32_t* mf, LgWin* win, int B, int H, int W, int search_mode, hipStream_t s, uint32_t init0 = 0xFFFFFFFFu);
int lg_launch_dt(bool bwd, const uint8_t* mask, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                 int H, int W, uint32_t init0, hipStream_t s);   // init0: lg_params.chamfer_init_dist0 (frames without a zero pixel)
// max d_out outside the sweep windows (closed-form chamfer norm on the frame border) -> atomicMax into maxfix[b][1]
void lg_launch_dout_border(const unsigned long long* bits, const LgWin* win, uint32_t* maxfix, int B, int H, int W, int WW,
                           hipStream_t s);

// ---- d_in without the row-sequential sweeps (frames with LgWin::search_in): horizontal run distances of the bounding-box rows
// into `tmp` (the d_in half of the sweep workspace, as uint16), then one form of the search over rows, which writes distance_map
// inside the window and the maximum into maxfix[b][0].  The numbering is LG_DT_SEARCH_ALGO's and lg_debug_dt_search_form's
// (2, 3 and 4 were the two-level search with recorded minimising rows: DESIGN.md).
enum {
    LG_DT_FORM_ROWS = 1,    // every row by the bounded search over rows: lg_launch_dt_rows
    LG_DT_FORM_BANDS = 5,   // pairs of adjacent seed rows by that search, the rows between two pairs by the chamfer stencil run
                            // down and up in registers: lg_launch_dt_seeds, then lg_launch_dt_bands.  H, W >= 16
    LG_DT_FORM_SWEEP = 6,   // the whole bounding box by that stencil, one workgroup per frame: lg_launch_dt_sweep.  H >= 16,
                            // 16 <= W <= 2048
};
// The form a batch of n frames of H x W takes; forced = LG_DT_SEARCH_ALGO (0: by size).  One level up to 64 frames of 1080p (one
// launch, the device is not full: 32 of 1080p 0.14 vs 0.18 ms).  Above, the register sweep when a bounding box's span fits 64
// lanes x 32 columns, W <= 2048: 256 of 1080p 0.229 ms against 0.235 + 0.140 for seed pairs + bands, and one workgroup per CU
// instead of 32 k workgroups beside the side chain (profiles/NOTES_dt_sweep.md); 4K keeps seed pairs + bands
// (profiles/NOTES_dt_bands.md).  The seed rows of form 5 share the run distances' workspace and need the room of sixteen rows
// and columns, form 6 likewise: lower or narrower frames take form 1 whatever is asked for.
inline int lg_dt_form(int forced, int n, int H, int W) {
    const bool bands_ok = H >= 16 && W >= 16, sweep_ok = bands_ok && W <= 2048;
    const int big = sweep_ok ? LG_DT_FORM_SWEEP : bands_ok ? LG_DT_FORM_BANDS : LG_DT_FORM_ROWS;
    switch (forced) {
        case LG_DT_FORM_ROWS: return LG_DT_FORM_ROWS;
        case LG_DT_FORM_BANDS: return bands_ok ? LG_DT_FORM_BANDS : LG_DT_FORM_ROWS;
        case LG_DT_FORM_SWEEP: return big;
        default: return (long long)n * H * W <= 64ll * 1080 * 1920 ? LG_DT_FORM_ROWS : big;
    }
}
void lg_launch_hrun(const unsigned long long* bits, uint32_t* tmp, const LgWin* win, int B, int H, int W, int WW, hipStream_t s);
void lg_launch_dt_rows(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                       int H, int W, int WW, hipStream_t s);
// band_p = 12 | 16 | 24 | 32 (else 16): rows from one seed pair to the next; band_e = 2 | 4: columns per lane of the band kernel
void lg_launch_dt_seeds(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, hipStream_t s);
void lg_launch_dt_bands(const unsigned long long* bits, uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B,
                        int H, int W, int WW, int band_p, int band_e, hipStream_t s);
void lg_launch_dt_sweep(uint32_t* tmp, float* dist_out, uint32_t* maxfix, const LgWin* win, int B, int H, int W, hipStream_t s);
