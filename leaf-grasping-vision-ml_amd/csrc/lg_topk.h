// Top-k and survivors (lg_topk.hip): the bound that prunes candidates in front of the CNN, and the launchers.
#pragma once
#include "lg_internal.h"

#include <math.h>

// true: a candidate with traditional score trad_i can never be taken by the selection loop (:226-236) of a frame whose
// candidate 0 has traditional score trad_0, whatever its logit -- its patch need not go through the CNN.  The loop starts
// from best = trad_0 and takes i only if comb_i > best, and best never falls.  ml lies in [0.5, 1]; maximising comb over ml:
//   trad_i <  0.5: w = 0.3 up to ml = 0.75, falling behind it      -> comb <= 0.7 trad_i + 0.225          (at ml = 0.75)
//   trad_i >= 0.5: w = 1.2 (1 - ml) behind 0.75, vertex (1 + t) / 2 -> comb <= trad_i + 0.3 (1 - trad_i)^2 (trad_i >= 1: comb <= trad_i)
// The margin covers the rounding of the float64 comb chain (a few ulp of 1 + |trad|; the margin is a thousand times that,
// float32 scores lie 6e-8 apart).  A NaN or an infinity in either score keeps the candidate.
__host__ __device__ inline bool lg_cnn_cannot_win(double trad_i, double trad_0) {
#pragma clang fp contract(off)
    if (!(fabs(trad_i) <= 1.7976931348623157e308) || !(fabs(trad_0) <= 1.7976931348623157e308)) return false;
    const double d = 1.0 - trad_i;
    const double ub = trad_i < 0.5 ? 0.7 * trad_i + 0.225 : trad_i + 0.3 * (d * d);
    const double margin = 1e-12 * (1.0 + fabs(trad_0) + fabs(trad_i));
    return ub + margin <= trad_0;
}

// tile_state (sparse planes, LgFinalArgs::sparse): [B][tiles] from lg_final_kernel, null when every plane was written.  The
// planes of a tile with state 0 were not written: top-k and the gather use the constant tile's values instead (flat_scale,
// w_flat: lg_params), computed with the operations of the final kernel's constant path.
// keep (needs out_info): [B] bit i = candidate i is scored by the rescoring and can still win (see lg_launch_survivors).
void lg_launch_topk(const float* trad, const uint8_t* valid, const float* depth, unsigned long long* tilekeys,
                    const uint8_t* tile_state, float flat_scale, float w_flat,
                    bool keys_ready, int B, int H, int W, int k, int min_dist, int32_t* out_xy, int32_t* out_n,
                    float* out_info, hipStream_t s, unsigned long long* keep = nullptr, int mask_is_bool = 0);

// Survivors of a batch (lg_launch_survivors, after lg_launch_topk with `keep`): keep[b] = bit i set when candidate i of frame
// b is scored by the rescoring (n > 1, border rule of a torch.bool mask) and can still win (lg_cnn_cannot_win).  list[j] =
// b * K + i of the j-th set bit in (frame, candidate) order, *count = their number, slot[b * K + i] = j or -1.  One workgroup;
// no atomics: the list is the same on every run.
void lg_launch_survivors(const unsigned long long* keep, int B, int K, int32_t* list, int32_t* slot, int32_t* count, hipStream_t s);
