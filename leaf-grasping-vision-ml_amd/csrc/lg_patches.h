// Patch windows (lg_patches.hip): the CNN's patch gather, training-sample harvesting, the negative-sample masks.
#pragma once
#include "lg_internal.h"

struct LgFinalArgs;   // lg_planes.h
struct LgIsoFields;   // lg_iso.h

// list / count (lg_launch_survivors; both null: every candidate): patch slot j takes entry list[j], slots >= *count are left alone
// defer (deferred planes; haloed patches, tile_state given): the arguments of the score-only lg_launch_final over the same
// frames.  Of maps_dev only flatness and distance are read then; sdf, approach, isolation, accessibility and stem of a window's
// pixels on a state-1 tile are computed here, by the plane kernel's own per-pixel code.
void lg_launch_gather(const float* depth, const uint8_t* mask, const float* const* maps_dev, const uint8_t* tile_state,
                      float flat_scale, int B, int H, int W, int k, const int32_t* xy, const int32_t* n, float* patches,
                      bool haloed, hipStream_t s, const int32_t* list = nullptr, const int32_t* count = nullptr,
                      const LgFinalArgs* defer = nullptr, const struct LgIsoFields* iso = nullptr);
void lg_launch_harvest(const float* depth, const uint8_t* mask, const float* const* maps_host, int H, int W, int n,
                       const int32_t* xy, const int32_t* rot, float* out_depth, float* out_mask, float* out_scores,
                       int32_t* flags, hipStream_t s);
void lg_launch_negative_masks(const float* dist, const uint8_t* mask, uint8_t* tip, uint8_t* stem, uint8_t* scratch, int H,
                              int W, hipStream_t s);
