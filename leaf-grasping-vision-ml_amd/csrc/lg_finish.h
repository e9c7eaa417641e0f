// The tail of select_grasp_point (lg_finish.hip): its arguments, the ranking of the candidates and the CNN's combined score as
// the device and the host exports run them, and the launchers.
#pragma once
#include "lg_internal.h"

#include <math.h>

// The host half of select_grasp_point on the device (lg_finish_kernel): CNN rescoring of the candidates, 3-D point, pre-grasp point
struct LgFinishArgs {
    const int32_t* cand_n;        // [B]
    const int32_t* cand_xy;       // [B][K][2]
    const float* cand_info;       // [B][K][2] traditional score, depth at the candidate
    const float* logits;          // [B][K] (read only when use_cnn); with `slot`: one per patch slot
    const int32_t* slot;          // [B][K] patch slot of a candidate, -1: pruned (lg_launch_survivors); null: slot = b * K + i
    int slot_frames;              //   slots count from the first patch of the candidate's sub-batch of this many frames
    const LgFrameParams* fp;      // [B] (theta)
    const unsigned long long* bits;   // [B][H][WW] mask bit rows
    const unsigned long long* bits2;  // null, or (label-aware mode) [B][H][WW] bit rows of the other leaves: the pre-grasp probes
                                      //   test bits | bits2 = every leaf of the label image
    lg_grasp_result* out;         // [B] DEVICE
    int B, H, W, WW, K, use_cnn, mask_is_bool;
    double cx, cy, f;
    LgSeSpans se;                 // (2 * pregrasp_clearance + 1) ellipse
};
void lg_launch_finish(const LgFinishArgs& a, hipStream_t s);
// Every candidate of every frame in rank order (lg_candidates_kernel, after lg_launch_finish on the same stream): rows [B][K]
void lg_launch_candidates(const LgFinishArgs& a, lg_grasp_candidate* rows, hipStream_t s);

// The reference's selection (grasp_point_selector.py:205-236) applied again to what is left after each pick: remaining = 0..n-1
// in candidate order; rank r starts from the first remaining candidate j with best score trad[j] and, when rescoring and more
// than one candidate remains, takes every scored remaining i with comb[i] > best (in candidate order); the pick leaves the
// list.  Rank 0 is the reference's grasp point.  Comparisons only, as written: a NaN never wins and a NaN start is never
// beaten.  n <= 64.  The device (lg_candidates_kernel) and the host export lg_rank_grasp_candidates run this code.
__host__ __device__ inline void lg_rank_candidates(const double* trad, const double* comb, const int32_t* scored, int n,
                                                   int rescoring, int32_t* order, double* pick, int32_t* by_ml) {
    unsigned long long left = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    for (int r = 0; r < n; r++) {
        const int j = __builtin_ctzll(left);
        int best = j, ml = 0;
        double bs = trad[j];                                   // :205-207
        if (rescoring && (left & (left - 1ull)) != 0ull)      // :210, len(candidates) > 1
            for (unsigned long long m = left; m; m &= m - 1ull) {
                const int i = __builtin_ctzll(m);
                if (scored[i] && comb[i] > bs) { bs = comb[i]; best = i; ml = 1; }   // :226-236
            }
        order[r] = best;
        pick[r] = bs;
        by_ml[r] = ml;
        left &= ~(1ull << best);
    }
}

// CNN rescoring of one candidate (grasp_point_selector.py:133-136, :222-226): ml = tanh(3 sigmoid(logit)) / 2 + 1/2, its
// confidence, weight and combined score, in float64 with fp contraction off.  lg_finish_kernel / lg_candidates_kernel
// (lg_ml_rescore) and the host export lg_ml_combined_score run this code.
__host__ __device__ inline void lg_ml_combine(double logit, double trad, double* ml_out, double* conf_out, double* comb_out) {
#pragma clang fp contract(off)
    const double sg = 1.0 / (1.0 + exp(-logit));
    const double ml = tanh(sg * 3.0) * 0.5 + 0.5;               // :133-136
    const double conf = 1.0 - fabs(ml - 0.5) * 2.0;              // :222
    const double wml = fmin(0.3, conf * 0.6);                    // :223
    *comb_out = (1.0 - wml) * trad + wml * ml;                   // :226
    *ml_out = ml;
    *conf_out = conf;
}
