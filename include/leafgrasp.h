/*
 * leafgrasp.h -- C-ABI of the MI355X (gfx950) grasp-scoring library, liblgrasp.so.
 *
 * Drop-in boundary for the per-pixel grasp-scoring hot path of
 * Srecharan/Leaf-Grasping-Vision-ML (reference paths are relative to the reference repo root).
 * Plain pointers and sizes only; no torch types.  All image pointers are DEVICE pointers owned by
 * the caller (e.g. torch tensor.data_ptr()); frames are dense row-major [B][H][W].
 * Every entry point returns 0 (LG_OK) or a negative lg_status; nothing throws, nothing exits.
 * One handle <-> one device; calls on one handle are stream-ordered, one at a time (a second thread entering the same
 * handle gets LG_ERR_BUSY); handles are independent -- threads may drive different handles concurrently -- and
 * the library keeps no global mutable state (SURVEY.md 8b "Threading").
 *
 * Reference interfaces replaced (what a ctypes/cffi binding in the reference would call):
 *   lg_score_maps      GraspPointSelector._calculate_all_scores + _get_valid_regions
 *                      (scripts/utils/grasp_point_selector.py:256-288) and everything they call:
 *                      calculate_sdf_score :526-567, calculate_approach_vector_score :569-593,
 *                      _calculate_flatness_map :635-657 + ImageProcessor.smooth_depth
 *                      (scripts/utils/image_processor.py:56-64), _calculate_isolation_score :595-633,
 *                      cv2.distanceTransform :266, _calculate_accessibility_score :502-524,
 *                      _calculate_stem_penalty :688-701, estimate_leaf_orientation :718-752
 *   lg_smooth_depth    ImageProcessor.smooth_depth (scripts/utils/image_processor.py:56-64)
 *   lg_topk_nms        GraspPointSelector._get_candidate_points  :447-482
 *   lg_gather_patches  get_ml_score feature assembly :59-127 + _extract_local_patch :392-445
 *   lg_cnn_load / lg_cnn_forward   GraspPointCNN.forward (eval)
 *                      (scripts/utils/ml_grasp_optimizer/model.py:101-128), load_ml_model :43-57
 *   lg_select_grasp    GraspPointSelector.select_grasp_point :184-253 (whole path, batched)
 *   lg_select_grasp_candidates   the per-candidate log lines of its selection loop :210-236, every candidate ranked
 *   lg_select_grasp_ml   the commented-out "grasp point based on only ML model" select_grasp_point :290-390 (batched)
 *   lg_select_grasp_collect   the select_grasp_point that calls collect_sample (scripts/utils/grasp_point_selector_bkp.py:73-169):
 *                      eroded safe zone, tip penalty, plain arg-max, centroid fallback (batched); lg_erode_ellipse, lg_tip_penalty
 *                      and lg_argmax_first are its stages on their own
 *   lg_harvest_patches / lg_negative_masks / lg_leaf_contour   EnhancedGraspDataCollector's patch extraction and
 *                      negative-region helpers (scripts/utils/ml_grasp_optimizer/data_collector.py:91-173,426-490)
 *   lg_leaf_stats      the per-leaf passes of OptimalLeafSelector.select_optimal_leaf
 *                      (scripts/utils/leaf_scorer.py:32-47,66-71,74-138)
 *   lg_clahe / lg_detect_midrib / lg_midrib_walk   GraspPointSelector.detect_midrib
 *                      (scripts/utils/grasp_point_selector.py:829-922), which LeafVisualizer calls
 *                      (scripts/utils/visualizer.py:141)
 *   lg_cnn_load_from_trainer / lg_cnn_evaluate / lg_eval_logits   the validation pass of train_grasp_model
 *                      (scripts/train_model.py:280-311: model.eval(), per-batch criterion, accuracy, analyze_predictions
 *                      :64-99) on the weights the training step has just written, without a trip through the host
 */
#ifndef LEAFGRASP_H
#define LEAFGRASP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_ctx* lg_handle;

typedef enum lg_status {
    LG_OK = 0,
    LG_ERR_INVALID = -1,  /* bad argument (null pointer, non-positive size, unsupported shape) */
    LG_ERR_HIP = -2,      /* a HIP runtime call failed; see lg_last_error */
    LG_ERR_NOMEM = -3,
    LG_ERR_NO_MODEL = -4, /* lg_cnn_forward without lg_cnn_load (reference: ml_predictor is None) */
    LG_ERR_UNSUPPORTED = -5,
    LG_ERR_BUSY = -6      /* another thread is inside a call on this handle (one call in flight per handle; the error string
                             of the running call is left alone) */
} lg_status;

/* Indices into out_maps[] -- the keys of the reference's `scores` dict
   (grasp_point_selector.py:258-280), in get_ml_score's channel order (:95-99) + traditional. */
enum {
    LG_MAP_SDF = 0,        /* 'sdf_score' */
    LG_MAP_APPROACH = 1,   /* 'approach_score' */
    LG_MAP_FLATNESS = 2,   /* 'flatness_map' */
    LG_MAP_ISOLATION = 3,  /* 'isolation_map' */
    LG_MAP_DISTANCE = 4,   /* 'distance_map' */
    LG_MAP_ACCESS = 5,     /* 'accessibility_map' */
    LG_MAP_STEM = 6,       /* 'stem_penalty' */
    LG_MAP_TRADITIONAL = 7,/* 'traditional_score' */
    LG_NUM_MAPS = 8
};

/* Every constant of the path; lg_default_params fills the reference values. */
typedef struct lg_params {
    double cx, cy, f;                /* camera: P[0,2], P[1,2], P[0,0]  (:145-150); defaults 707, 494, 0 (unset).
                                        double: x - cx cancels catastrophically in float32 next to the optical centre */
    float w_approach, w_sdf, w_flat, w_access;      /* 0.4 0.3 0.2 0.1            (:272-277) */
    float sdf_w_interior, sdf_w_align, sdf_w_sdf;   /* 0.4 0.4 0.2                (:563-565) */
    float optimal_distance;                         /* 20 px                      (:535-536) */
    float access_w_dist, access_w_dir;              /* 0.7 0.3                    (:522)     */
    float flat_scale;                               /* 5                          (:655)     */
    float iso_w_close, iso_w_wide;                  /* 0.7 0.3                    (:620)     */
    float iso_ramp_top, iso_ramp_bottom;            /* 1.0 0.2                    (:623)     */
    float min_edge_distance;                        /* 20                         (:25,285)  */
    float stem_valid_thresh;                        /* 0.8                        (:287)     */
    int32_t stem_se;                                /* ellipse 30                 (:696); 1..64 */
    int32_t stem_bottom_div;                        /* bottom H//3 rows           (:693); >= 1.  A divisor larger than H follows
                                                       numpy as the reference's line does: H // div == 0 and bottom[-0:, :] is the
                                                       WHOLE frame, so every leaf pixel is stem (not "no row") */
    int32_t top_k;                                  /* 20                         (:197)     */
    int32_t nms_min_distance;                       /* 10                         (:198)     */
    int32_t pregrasp_clearance;                     /* 15 px (SE 31)              (:777-778) */
    int32_t mask_is_bool;                           /* 1: torch.bool mask => border patches give no ML score */
    int32_t gaussian_size;                          /* 5: the ImageProcessor's smoothing kernel that _calculate_flatness_map applies
                                                       (:635-657, image_processor.py:25-32,56-64; sigma = size / 6).  1, 3, 5, 7;
                                                       anything else => LG_ERR_UNSUPPORTED (an even size raises in the reference) */
    int32_t chamfer_init_dist0;                     /* OpenCV's INIT_DIST0, the value cv2.distanceTransform's border cells start from.
                                                       It shows in the transform of an image WITHOUT any zero pixel, which is
                                                       what _calculate_isolation_score asks for (:605-616: other_leaves == 0) and
                                                       what dist_inside of an all-ones mask is: INIT_DIST0 / 65536 + weight * (distance
                                                       to the frame) -- and, as a cap of that form on every pixel, in a frame where
                                                       a chamfer distance can reach it (INT_MAX >> 2 is 8192 px: 16384 rows, or 8192
                                                       columns; such a frame is swept whole).  A value above INT_MAX >> 2 is refused
                                                       (LG_ERR_UNSUPPORTED) on a frame whose diagonal norm reaches 16384 px.  The constant depends on the OpenCV revision: INT_MAX >> 2
                                                       (536870911, default; distransform.cpp of the 2.4 / 3.x lines) or INT_MAX
                                                       (2147483647; revisions that lifted the 8192-pixel ceiling).  The pinned
                                                       opencv-python 4.10.0.84 is absent here: parity unpinned.
                                                       Range [INT_MAX >> 2, INT_MAX] */
    int32_t label_aware;                            /* 0 (default): the reference as written -- _calculate_isolation_score and
                                                       calculate_pre_grasp_point see the one leaf they were handed (DESIGN 2 quirks 1
                                                       and 14).  1: both see the OTHER leaves of the label image, as their comments
                                                       promise; only lg_select_grasp_labels / lg_select_grasp_candidates_labels take
                                                       it (see there), every entry without a label image returns LG_ERR_INVALID.
                                                       Any other value: LG_ERR_INVALID */
} lg_params;

/* Raw GraspPointCNN(in_channels=9, attention_type, encoder_filters) state_dict tensors, HOST pointers,
   float32, PyTorch layouts (conv: [Cout][Cin][3][3], linear: [out][in]); BN is folded at load.
   attention_type (scripts/utils/ml_grasp_optimizer/model.py:30-60): LG_ATT_SPATIAL is what the node
   instantiates (grasp_point_selector.py:40); CHANNEL / HYBRID / NONE are the sweep variants. */
enum { LG_ATT_SPATIAL = 0, LG_ATT_CHANNEL = 1, LG_ATT_HYBRID = 2, LG_ATT_NONE = 3 };
typedef struct lg_cnn_weights {
    const float* conv_w[8];  const float* conv_b[8];       /* encoder.{b}.{0,3}, b < n_blocks (2 per block) */
    const float* bn_g[8]; const float* bn_b[8]; const float* bn_m[8]; const float* bn_v[8]; /* encoder.{b}.{1,4} */
    const float* att_w; const float* att_b;               /* attention.0 : [1][256][1][1], [1] */
    const float* fc_w[4]; const float* fc_b[4];            /* classifier.{0,4,8,12} */
    const float* fbn_g[3]; const float* fbn_b[3]; const float* fbn_m[3]; const float* fbn_v[3]; /* classifier.{1,5,9} */
    float bn_eps;                                          /* 1e-5 */
    int32_t attention_type;                                /* LG_ATT_*; att_w/att_b: SPATIAL, HYBRID (spatial_attention.0) */
    const float* ca_w1; const float* ca_b1;                /* CHANNEL: attention.1, HYBRID: channel_attention.1 : [16][256][1][1], [16] */
    const float* ca_w2; const float* ca_b2;                /*          attention.3,         channel_attention.3 : [256][16][1][1], [256] */
    int32_t n_blocks;                                      /* 0 = the default encoder [64,128,256]; else 3 or 4 */
    int32_t filters[4];                                    /* encoder_filters: [32,64,128] [64,128,256] [64,128,256,512] [128,256,512]
                                                              (train_model_mlflow.py:177-182); attention / classifier sizes follow filters[n_blocks-1] */
} lg_cnn_weights;

/* Per-frame result of lg_select_grasp (HOST memory). */
typedef struct lg_grasp_result {
    int32_t found;            /* 0 => reference returns (None, None, None) */
    int32_t x, y;             /* grasp_point_2d */
    float   X, Y, Z;          /* grasp_point_3d   (:152-180) */
    int32_t has_pre;          /* pre-grasp point present */
    float   pX, pY, pZ;       /* pre_grasp_point  (:754-819) */
    int32_t n_candidates;
    int32_t ml_used;          /* a CNN-rescored candidate replaced the best traditional one */
    float   best_score;
    float   theta;            /* leaf orientation (rad), NaN if none */
} lg_grasp_result;

/* One candidate of lg_select_grasp_candidates (HOST memory), in rank order: the reference's selection
   (:205-236) applied again to the candidates left after each pick.  17 four-byte fields, 68 bytes. */
typedef struct lg_grasp_candidate {
    int32_t index;            /* position in the candidate list (_get_candidate_points :447-482); -1 = unused row (all else 0) */
    int32_t x, y;             /* the candidate pixel */
    float   traditional;      /* traditional_score there (:205, :213) */
    float   ml_score;         /* get_ml_score (:133-136)          NaN when not scored */
    float   ml_confidence;    /* 1 - |ml - 0.5| * 2 (:222)        NaN when not scored */
    float   combined;         /* (1 - w) trad + w ml (:223-226)   NaN when not scored */
    int32_t scored;           /* the reference computes a combined score for it (CNN loaded, n > 1, not a border
                                 candidate of a torch.bool mask: SURVEY App. B.7) */
    float   pick_score;       /* the score that decided this rank (rank 0: lg_grasp_result.best_score) */
    int32_t by_ml;            /* a combined score decided it (rank 0: lg_grasp_result.ml_used) */
    float   X, Y, Z;          /* get_3d_grasp_point (:152-180) */
    int32_t has_pre;          /* pre-grasp point present */
    float   pX, pY, pZ;       /* calculate_pre_grasp_point (:754-819) */
} lg_grasp_candidate;

/* Per-leaf statistics of lg_leaf_stats (HOST memory), one per label id present, ascending id. */
typedef struct lg_leaf_stat {
    int32_t id;
    int32_t area;             /* pixel count                          (leaf_scorer.py:79) */
    int32_t touches_border;   /* any pixel on the image border        (:286-291) */
    int32_t pad_;
    double  sum_x, sum_y;     /* centroid numerators                  (:84-88)   */
    double  sum_depth;        /* mean depth numerator                 (:105-106) */
    double  sum_ray;          /* sum over pixels of sqrt((x-cx)^2+(y-cy)^2+f^2)  (:109-115) */
    float   median_depth;     /* np.median of the leaf's depths       (:41-47)   */
    float   pad2_;
} lg_leaf_stat;

int lg_create(int device, lg_handle* out);
int lg_destroy(lg_handle h);
const char* lg_last_error(lg_handle h);
/* "" normally; why the device-side contour analysis (estimate_leaf_orientation, :718-752) could not be set up for this handle's
   workspace -- scoring then goes on with the host analysis of every frame (same results). */
const char* lg_orientation_note(lg_handle h);
const char* lg_version(void);
void lg_default_params(lg_params* p);

/* Score planes for B frames.  depth [B][H][W] f32, mask [B][H][W] u8 (0/1), out_maps[i] [B][H][W] f32
   (any entry may be NULL = not wanted, DISTANCE and TRADITIONAL included: later stages need those two, so the call
   computes them into planes of the handle's workspace instead and goes on; out_maps itself may be NULL = no plane wanted),
   out_valid [B][H][W] u8 (may be NULL: a workspace plane takes its place).  Every subset gives the planes it asks for
   within the library's tolerances; flatness and traditional of a call that leaves out a plane other than those two may
   differ in the last bit from a call that takes all eight.  theta_host (optional, HOST, B floats) receives the leaf
   axis angle per frame (NaN when the mask has no contour).  Work is enqueued on `stream`
   (a hipStream_t, NULL = default stream); the call synchronises internally only with its own
   copy stream (orientation hand-off), not with `stream`. */
int lg_score_maps(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W,
                  const lg_params* p, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                  float* theta_host, void* stream);

/* ImageProcessor.smooth_depth (scripts/utils/image_processor.py:56-64) on its own: reflect padding by gaussian_size / 2, then
   the gaussian_size x gaussian_size kernel of _create_gaussian_kernel (:25-32, sigma = size / 6) applied as its two 1-D
   factors.  depth [B][H][W] f32 DEVICE -> out [B][Ho][Wo] f32 DEVICE, Ho = H + 2 (size / 2) - size + 1 (= H for odd sizes,
   H + 1 for even ones, as F.conv2d returns); 1 <= gaussian_size <= 15, gaussian_size / 2 < min(H, W).
   Stateless: only the handle's device is used and nothing of the handle is written, so threads may share a handle here (it takes
   no part in the one-call-in-flight rule); the reason of a failure is per thread: lg_last_error(NULL).
   lg_gaussian_taps: that 1-D factor (HOST, gaussian_size floats) -- what the plane kernel and lg_smooth_depth multiply with. */
int lg_smooth_depth(lg_handle h, const float* depth, int B, int H, int W, int gaussian_size, float* out, void* stream);
int lg_gaussian_taps(int gaussian_size, float* taps);

/* Greedy spaced top-k on valid_scores = trad*valid (score desc, flat index desc on ties).
   out_xy [B][k][2] int32 (x,y) DEVICE, out_n [B] int32 DEVICE. */
int lg_topk_nms(lg_handle h, const float* trad, const uint8_t* valid, int B, int H, int W, int k,
                int min_dist, int32_t* out_xy, int32_t* out_n, void* stream);

/* 9-channel 32x32 patches around n_xy points per frame.  maps[] as produced by lg_score_maps
   (indices 0..6 are read).  xy [B][k][2] DEVICE, n [B] DEVICE; patches [B][k][9][32][32] f32 DEVICE.
   Depth and the seven planes are min-max normalised per window where max > min, by numpy's rules: a channel whose window
   holds a NaN has a NaN minimum and maximum and stays raw (the NaN included); one that holds an infinity is divided by an
   infinite range (0 at its finite pixels, NaN at the infinite ones).  Depth is read as passed, off the leaf too. */
int lg_gather_patches(lg_handle h, const float* depth, const uint8_t* mask,
                      const float* const maps[LG_NUM_MAPS], int B, int H, int W, int k,
                      const int32_t* xy, const int32_t* n, float* patches, void* stream);

int lg_cnn_load(lg_handle h, const lg_cnn_weights* w);
int lg_cnn_unload(lg_handle h);
/* patches [N][9][32][32] f32 DEVICE -> logits [N] f32 DEVICE.
   Every ReLU and max-pool propagates NaN as torch's relu and max_pool2d do: a patch that holds a NaN or an infinity in any
   channel gets a NaN logit (and through lg_ml_combined_score a NaN ml score, confidence and combined score, which never wins
   the selection); the other patches of the call are computed as if it held finite values, bit for bit. */
int lg_cnn_forward(lg_handle h, const float* patches, int N, float* logits, void* stream);

/* Whole GraspPointSelector.select_grasp_point for B frames: maps -> valid -> top-k -> (CNN rescoring
   if a model is loaded) -> 3-D point -> pre-grasp.  out_maps / out_valid may be NULL, and so may any entry of out_maps, as
   for lg_score_maps (library workspace is used for what is left out; the result rows name the same grasp pixel whichever
   subset is taken back).  results: HOST array of B.  Synchronises `stream` before returning. */
int lg_select_grasp(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W,
                    const lg_params* p, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                    lg_grasp_result* results, void* stream);

/* lg_select_grasp on mask[b] = (labels[b] == leaf_ids[b]): the node's `optimal_mask = mask_tensor == optimal_leaf_id` followed
   by select_grasp_point (scripts/leaf_grasp_node_v3.py:118-125) with the comparison folded into the library's first pass over
   the frame.  labels [B][H][W] int16 DEVICE (the label image lg_leaf_select_batch reads), leaf_ids [B] HOST (an id no label
   carries, e.g. INT32_MIN, gives that frame an empty mask and found = 0).  Everything else as lg_select_grasp; the node's mask
   is a torch.bool tensor: set lg_params.mask_is_bool = 1 for its behaviour at the image border.
   lg_params.label_aware = 1 (opt-in; 0 leaves every result as it was).  Per frame, with id = leaf_ids[b], current = (labels ==
   id), others = (labels > 0) & (labels != id) (a negative label is background) and all = labels > 0:
     isolation plane (:605-627 with `other_leaves` = others): ic / iw = others dilated by the 30 / 40 ellipses (anchor k / 2,
       outside the frame = 0), dc / dw = cv2.distanceTransform(1 - ic / 1 - iw, DIST_L2, 3) in exact 16.16 integers, each
       divided by its own whole-frame maximum + 1e-6 in float32, iso_w_close * sc + iso_w_wide * sw, times the height ramp,
       times current.  A frame whose `others` is empty keeps the closed-form plane of label_aware = 0, bit for bit.
     pre-grasp clearance (:786-815): the five probes test dilate(all, ellipse 2 * pregrasp_clearance + 1) instead of the
       dilated current leaf -- the result row's and every ranked candidate's pre-grasp point.
   Traditional score, validity, the candidates and the 3-D point do not read either.  The CNN sees the new channel 5: ml_score,
   combined and the pick may change -- a model trained on the degenerate channel should be retrained on patches collected in
   this mode.  Workspace for the mode is allocated by the first call that sets it. */
int lg_select_grasp_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W,
                           const lg_params* p, float* const out_maps[LG_NUM_MAPS], uint8_t* out_valid,
                           lg_grasp_result* results, void* stream);

/* Every candidate of every frame, ranked: the selection loop of select_grasp_point (:205-236, which logs each candidate's
   scores) applied again to what is left after each pick, so rank 1 is the grasp the reference would choose if rank 0 were
   taken away.  results: as lg_select_grasp / lg_select_grasp_labels fill them.  cands: HOST array of B * p->top_k rows,
   frame after frame, in rank order; rows past n_candidates have index = -1 and zeros elsewhere.  No plane outputs.  The
   rows are computed on the device in double precision (the ranking compares the unrounded combined scores). */
int lg_select_grasp_candidates(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* p,
                               lg_grasp_result* results, lg_grasp_candidate* cands, void* stream);
int lg_select_grasp_candidates_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B,
                                      int H, int W, const lg_params* p, lg_grasp_result* results, lg_grasp_candidate* cands,
                                      void* stream);
/* The ranking alone on the host (no device, no handle) for ONE frame of n <= 64 candidates: trad[n], comb[n], scored[n] as
   the device computes them (comb is read only where scored), rescoring = a CNN is loaded and n > 1.  order[n]: candidate
   indices in rank order; pick[n], by_ml[n]: the deciding score and whether a combined score decided.  The device runs this code. */
int lg_rank_grasp_candidates(const double* trad, const double* comb, const int32_t* scored, int n, int rescoring,
                             int32_t* order, double* pick, int32_t* by_ml);

/* The CNN rescoring of one candidate on the host (no device, no handle), the code the device runs (:133-136, :222-226):
   ml = tanh(3 sigmoid(logit)) / 2 + 1/2, confidence = 1 - 2 |ml - 1/2|, combined = (1 - w) trad + w ml, w = min(0.3, 0.6 confidence).
   lg_cnn_candidate_cannot_win: 1 if a candidate with traditional score trad_i can never be taken by the selection loop of a
   frame whose candidate 0 scores trad_0, whatever its logit -- combined <= 0.7 trad_i + 0.225 (trad_i < 0.5), <= trad_i +
   0.3 (1 - trad_i)^2 (else), compared with a margin of 1e-12 (1 + |trad_0| + |trad_i|); 0 for a NaN or an infinity in either
   score.  lg_select_grasp does not put such a candidate's patch through the CNN (LG_CNN_PRUNE=0 at lg_create: it does). */
int lg_ml_combined_score(double logit, double trad, double* ml, double* confidence, double* combined);
int lg_cnn_candidate_cannot_win(double trad_i, double trad_0);

/* ---- ML-only grasp selection: the "grasp point based on only ML model" form of select_grasp_point that the reference keeps
   commented out beside the live one (scripts/utils/grasp_point_selector.py:290-390): the seven planes, a walk over the leaf's
   pixels, GraspPointCNN on each sampled pixel's 32 x 32 window, the best score -- or the mask centroid when nothing could be
   scored.  Per frame, n = the number of set mask pixels; sample order is row-major (np.where order).
   Sampling  LG_ML_SAMPLE_NTH (the reference's, :310-320): step = max(1, n / target) in integers, the samples are leaf pixels
             number 0, step, 2 step, ... below n -- at most 2 target - 1 of them (max_samples must hold that many).
             LG_ML_SAMPLE_GRID (the score as a map over the leaf): the leaf pixels with x % stride == 0 && y % stride == 0,
             stride in 1..64.  A frame with more such pixels than max_samples overflows: found = 0, n_samples[b] = -(their
             number), no rows; the other frames of the call are unaffected and the call returns LG_OK.
             max_samples in 1..65536 is the row length of `samples`; chunk in 0..8192 = patches per gather + CNN pass (0:
             the library's default, 1024) -- results do not depend on it.
   Border    (:326-328, both modes) a sample with y < 16 || y >= H - 16 || x < 16 || x >= W - 16 stays in the table with scored
             = 0 and is not put through the CNN.  This is the commented code's rule, not get_ml_score's torch.bool rule: x ==
             W - 16 is skipped here and lg_params.mask_is_bool plays no part.  A scored window never needs replicate padding.
   Features  those of the live get_ml_score (:59-143), i.e. what lg_gather_patches and lg_cnn_forward compute: min-max
             normalisation per window, the raw mask channel, NaN propagation as lg_cnn_forward documents it.  The commented
             block's un-normalised patches are not reproduced.
   Values    logit, and ml_score = lg_ml_combined_score's ml = tanh(3 sigmoid(logit)) / 2 + 1/2 rounded to float.  scored = 1: the
             sample went through the CNN (no model loaded: every row has scored = 0).  Unscored rows carry NaN in both; rows
             past the frame's samples are zeros.
   Pick      the first sample in order whose logit is strictly greater than every earlier scored sample's (:364, score >
             best_score): the first occurrence of the largest logit.  A NaN logit never wins.  The reference compares the
             float32 sigmoid; the logit orders the samples the same way except where that sigmoid saturates or two logits
             collide in it, where the reference keeps the earlier sample and this keeps the larger logit.
   Fallback  (:368-378) no model loaded, no scored sample, or only NaN logits: the pick is the centroid (sum x / n, sum y / n),
             truncated, from exact 64-bit integer sums (torch's float32 mean() may round differently on a large leaf); ml_used
             = 0, best_score = NaN.  Empty mask: found = 0 (the reference's int(nan) raises and ends in its None triple).
   Result    x, y = the pick; X, Y, Z, has_pre, pX, pY, pZ by the code lg_select_grasp runs for its pick; n_candidates = the
             samples that went through the CNN; ml_used = 1: a CNN score picked; best_score = the pick's ml_score or NaN;
             theta as lg_select_grasp.
   lg_select_grasp_ml_labels: mask[b] = labels[b] == leaf_ids[b] as lg_select_grasp_labels; lg_params.label_aware passes
   through as there (channel 5 and the pre-grasp clearance); lg_select_grasp_ml rejects it (lg_label_aware_check).
   samples: HOST [B][max_samples] or NULL; n_samples: HOST [B] or NULL.  Synchronises `stream` before returning.  The device
   builds the table from the mask's bit rows without atomics: it is the same on every run and equals
   lg_ml_sample_points_host's, which runs the same code on the host (no device, no handle): xy [cap][2], scored [cap], *n = the
   samples (GRID with more than min(cap, max_samples) of them: -(their number), nothing written), sums = {sum x, sum y, area}
   over the set pixels; any output pointer but n may be NULL.  LG_ERR_INVALID for a bad argument, NTH included when min(cap,
   max_samples) < 2 target - 1. */
enum { LG_ML_SAMPLE_NTH = 0, LG_ML_SAMPLE_GRID = 1 };
typedef struct lg_ml_sampling {
    int32_t mode, target, stride, max_samples, chunk;   /* chunk: patches per gather+CNN pass, 0 = library default */
} lg_ml_sampling;
typedef struct lg_ml_sample {
    int32_t x, y, scored;
    float logit, ml_score;
} lg_ml_sample;   /* 20 bytes */
/* NTH, target 100, stride 8, max_samples 4096, chunk 0 */
void lg_default_ml_sampling(lg_ml_sampling* s);
int lg_select_grasp_ml(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* p,
                       const lg_ml_sampling* sampling, lg_grasp_result* results, lg_ml_sample* samples, int32_t* n_samples,
                       void* stream);
int lg_select_grasp_ml_labels(lg_handle h, const float* depth, const int16_t* labels, const int32_t* leaf_ids, int B, int H, int W,
                              const lg_params* p, const lg_ml_sampling* sampling, lg_grasp_result* results, lg_ml_sample* samples,
                              int32_t* n_samples, void* stream);
int lg_ml_sample_points_host(const uint64_t* bits, int H, int W, int WW, const lg_ml_sampling* sampling, int32_t* xy,
                             int32_t* scored, int cap, int32_t* n, int64_t sums[3]);
/* Where the gather of lg_select_grasp_ml* finds the five planes it does not read from the plane kernel's stores: form 1 = it
   computes them at the pixels of every window (deferred planes, what lg_select_grasp does), 2 = the plane kernel stores all
   seven on the leaf's tiles once and the gather reads them; 0 = by the library's rule (form 1; profiles/NOTES_ml_select.md has the
   measurement; LG_DEFER_PLANES=0 at lg_create: form 2).  Holds for the handle's later calls.
   *last (may be NULL) = the form the last lg_select_grasp_ml* call on this handle took, 0: none yet.  Same results either way. */
int lg_debug_ml_planes(lg_handle h, int form, int32_t* last);

/* ---- the collecting selector: the select_grasp_point that feeds the data collector (scripts/utils/grasp_point_selector_bkp.py
   :73-169, "bkp" below; the only caller of collect_sample in the reference).  DESIGN 2 quirk 16 has the details.  Per frame:
     safe      cv2.erode(mask, ellipse(erosion_kernel_size), iterations = erosion_iterations) (bkp:79-82); the frame border does
               not erode.
     planes    sdf, approach, isolation, distance, accessibility, stem and the leaf angle on `safe`; flatness on depth * the
               ORIGINAL mask (bkp:88-89), a whole-frame plane.
     tip       the tip penalty as written (bkp:395-408): `(~tip_area).astype(np.uint8)` has no zero pixel, so its 5 x 5 transform is
               chamfer_init_dist0 + 65536 min(x + 1, y + 1, W - x, H - y) in 16.16 integers; penalty = (1 - d / (max d + 1e-6)) on
               `safe`, 0 elsewhere (float32, as the isolation plane).  A ramp of a few per cent from the frame border.
     fusion    trad = float32(w_approach approach + w_sdf sdf + w_flat flatness + w_tip (1 - tip)) (1 - stem) valid, valid =
               (distance > min_edge_distance) & safe (bkp:98-108): no accessibility term, no stem threshold.  The sum is taken in
               double from the float32 planes.  Outside the bounding box of `safe` both are exactly 0.
     point     any trad > 0: np.argmax(trad), the first maximum in row-major order, a NaN counting as the maximum; else the
               centroid of the ORIGINAL mask, sum x / n and sum y / n in double from integer sums, rounded to float32, truncated
               (torch's float32 mean may differ from that in the last bit: DESIGN).  Empty original mask: found = 0.
     result    x, y = the point; X, Y, Z, has_pre, pX, pY, pZ by the code lg_select_grasp runs for its pick, the pre-grasp probes
               on dilate(safe, ellipse 2 pregrasp_clearance + 1) (bkp:82 reassigns the mask); n_candidates 1 for an arg-max
               point, 0 for the centroid; best_score = np.max(trad); theta = the angle of `safe`; ml_used 0.
   lg_params here: w_approach, w_sdf, w_flat the three weights, min_edge_distance the 20; w_access, stem_valid_thresh, top_k are not
   read; label_aware = 1 is LG_ERR_INVALID.  lg_collect_params: NULL = the defaults.  tip_aware = 1 (the method's stated intent: the
   transform of the tip area itself) is not built: LG_ERR_UNSUPPORTED.
   lg_collect_params_check (no device, no handle): the rule every entry below applies to the two structs (either may be NULL =
   defaults) -- LG_ERR_UNSUPPORTED for an even or out-of-range erosion_kernel_size (1..63), erosion_iterations outside 0..8,
   tip_aware = 1, and with it a tip_se that is even or outside 3..63; LG_ERR_INVALID for any other tip_aware and for label_aware != 0.
   lg_erode_ellipse        safe alone: mask, out u8 [B][H][W] DEVICE (0 / 1; nonzero mask bytes count as 1).  Enqueued on `stream`.
   lg_erode_words_host     the same on the host (no device, no handle) for one frame of bit rows [H][WW] (bit j of word w = pixel
                           64 w + j; bits past W are ignored and come out 0) -- the per-word code of the device.
   lg_tip_penalty          the tip plane alone on a given `safe` (u8, DEVICE): out f32 [B][H][W]; out_tip_area u8 [B][H][W] or NULL,
                           zeros unless tip_aware.  p: NULL = defaults (chamfer_init_dist0 is read).  Enqueued on `stream`.
   lg_tip_fix_host         the 16.16 field of the tip penalty as written over a whole H x W frame (no device, no handle), and its
                           maximum in *max_fix (may be NULL): what the device evaluates on the pixels of `safe`.
   lg_argmax_first         per frame of a handed plane f32 [B][H][W] DEVICE: xy_host [B][2] = np.argmax as (x, y), max_host [B] =
                           np.max (NaN when the plane holds one), any_positive_host [B] = (plane > 0).any(); each may be NULL.
                           Synchronises `stream`.
   lg_select_grasp_collect the whole of it.  out_maps[i] (any may be NULL, and out_maps itself), out_tip f32, out_safe u8, out_valid
                           u8: [B][H][W] DEVICE or NULL; out_maps[LG_MAP_TRADITIONAL] is the fused plane above.  The result rows do
                           not depend on which outputs are taken.  results: HOST array of B.  Synchronises `stream`. */
typedef struct lg_collect_params {
    int32_t erosion_kernel_size;  /* 21 (bkp:30); odd, 1..63 */
    int32_t erosion_iterations;   /* 2  (bkp:31); 0..8 */
    int32_t tip_se;               /* 15 (bkp:397); odd, 3..63; read only when tip_aware */
    int32_t tip_aware;            /* 0 as written, 1 intent; else LG_ERR_INVALID */
    float   w_tip;                /* 0.1 (bkp:102) */
} lg_collect_params;
void lg_default_collect_params(lg_collect_params* p);
int lg_collect_params_check(const lg_params* p, const lg_collect_params* cp);
int lg_erode_ellipse(lg_handle h, const uint8_t* mask, int B, int H, int W, int k, int iterations, uint8_t* out, void* stream);
int lg_erode_words_host(const uint64_t* bits, int H, int W, int WW, int k, int iterations, uint64_t* out);
int lg_tip_penalty(lg_handle h, const uint8_t* safe, int B, int H, int W, const lg_params* p, const lg_collect_params* cp, float* out,
                   uint8_t* out_tip_area, void* stream);
int lg_tip_fix_host(int H, int W, int32_t chamfer_init_dist0, uint32_t* out, uint32_t* max_fix);
int lg_argmax_first(lg_handle h, const float* plane, int B, int H, int W, int32_t* xy_host, float* max_host,
                    int32_t* any_positive_host, void* stream);
int lg_select_grasp_collect(lg_handle h, const float* depth, const uint8_t* mask, int B, int H, int W, const lg_params* p,
                            const lg_collect_params* cp, float* const out_maps[LG_NUM_MAPS], float* out_tip, uint8_t* out_safe,
                            uint8_t* out_valid, lg_grasp_result* results, void* stream);

/* The node's result message of every frame (leaf_grasp_node_v3.py:170-176: "x,y,X,Y,Z[,pX,pY,pZ]", each number as Python's
   str() prints it -- the shortest decimal string of the float32 value as a double), '\n'-terminated, one line per frame in
   order, an empty line for a frame without a result.  buf: HOST, cap bytes (>= 256 per frame); *used = bytes written.
   No device work; needs no handle. */
int lg_format_grasp_results(const lg_grasp_result* results, int n, char* buf, int64_t cap, int64_t* used);

/* Per-label statistics + clutter extrema for one frame.  labels [H][W] int16 DEVICE, depth DEVICE.
   stats: HOST array of capacity max_leaves; n_leaves: HOST.  extrema (HOST, 4 ints): first leaf
   pixel (y,x) and the background pixel farthest (exact Euclidean) from any leaf (y,x). */
int lg_leaf_stats(lg_handle h, const int16_t* labels, const float* depth, int H, int W,
                  float cx, float cy, float f, lg_leaf_stat* stats, int max_leaves, int* n_leaves,
                  int32_t* extrema, void* stream);
/* The same for B frames per call: labels / depth [B][H][W] DEVICE; stats [B][max_leaves], n_leaves [B], extrema [B][4],
   status [B] HOST (per-frame lg_status: a frame with more than 1024 labels fails alone with LG_ERR_UNSUPPORTED; one with more
   than max_leaves labels with LG_ERR_INVALID and its label count in n_leaves, so the caller can come back with room).  Every pass carries the frame
   in its grid; there is no host round trip between the passes. */
int lg_leaf_stats_batch(lg_handle h, const int16_t* labels, const float* depth, int B, int H, int W, float cx, float cy,
                        float f, lg_leaf_stat* stats, int max_leaves, int* n_leaves, int32_t* extrema, int* status,
                        void* stream);

/* OptimalLeafSelector.select_optimal_leaf (scripts/utils/leaf_scorer.py:25-203) for B frames, the whole of it: the per-leaf
   passes of lg_leaf_stats_batch and then, on the host inside the library, tall-leaf split, scores, Pareto filter and weighted
   pick.  ids [B] HOST: the chosen label (-1: the reference's None; -2: a frame with more than 256 labels or 128 leaves -- take
   it through lg_leaf_stats + the caller's own selection); n_tall [B], tall [B][tall_cap] HOST: get_tall_leaves() per frame. */
int lg_leaf_select_batch(lg_handle h, const int16_t* labels, const float* depth, int B, int H, int W, double cx, double cy,
                         double f, int32_t* ids, int32_t* n_tall, int32_t* tall, int tall_cap, void* stream);

/* The host half of lg_leaf_select_batch on its own (no device, no handle): the selection of leaf_scorer.py:53-203 from the rows
   of lg_leaf_stats for ONE frame -- mean of medians -> tall leaves, the three scores of every candidate with area >= 10000,
   Pareto filter on the tall (x 1.1) or the regular set, weighted pick.  *id: the chosen label, -1 = the reference's None, -2 =
   128 or more leaves (numpy's summation order of the float32 mean changes there: the caller's own path decides).  tall
   [tall_cap], *n_tall: get_tall_leaves() (*n_tall may exceed tall_cap; only tall_cap ids are written). */
int lg_leaf_select_from_stats(const lg_leaf_stat* stats, int n, const int32_t* extrema, int H, int W, double cx, double cy,
                              double f, int32_t* id, int32_t* tall, int tall_cap, int32_t* n_tall);

/* GraspPointSelector.estimate_leaf_orientation (:718-752) for one frame: mask [H][W] u8 DEVICE.
   out (HOST, 5 floats): angle (rad, direction of the longer side of the min-area rectangle of the largest
   outer contour, in (0, pi]), major axis, minor axis, centre x, centre y.  Returns LG_OK and *found = 0
   when the mask is empty.  Synchronises `stream`. */
int lg_leaf_orientation(lg_handle h, const uint8_t* mask, int H, int W, float* out, int* found, void* stream);

/* ---- GraspPointSelector.detect_midrib (:829-922)
   lg_clahe          cv2.createCLAHE(clipLimit=clip_limit, tileGridSize=(tiles_x, tiles_y)).apply on B gray frames (:842-843 on its
                     own; OpenCV clahe.cpp): src, dst u8 [B][H][W] DEVICE.  tiles 1..64 each, H, W >= 2, else LG_ERR_INVALID.
                     Sizes that do not divide by the tile counts pad BOTH dimensions at the end by tiles - size % tiles
                     (BORDER_REFLECT_101) for the histograms; clip_limit <= 0: no clipping.  Enqueued on `stream`.
   lg_detect_midrib  the whole method for B frames: leaf_region = image & mask (:834), COLOR_BGR2GRAY on channel indices 0, 1, 2
                     (:837; the visualiser hands in RGB, visualizer.py:133), CLAHE(3.0, (8, 8)) of the whole frame (:842-843),
                     estimate_leaf_orientation (:858, the values lg_leaf_orientation reports, as float32) and the ridge walk
                     (:864-907).  image u8 [B][H][W][C] DEVICE, C = 3 or 4 (the fourth byte is ignored, as BGR2GRAY ignores
                     alpha); mask u8 [B][H][W] DEVICE (nonzero = leaf).  out [B][4] HOST: x0, y0, x1, y1 (the first and the last
                     ridge point); status [B] HOST: 0 found, 1 no contour, 2 int(minor / 6) == 0 (cv2.line asserts thickness > 0:
                     the reference logs an error and returns None), 3 fewer than two ridge points (None); out is -1 unless 0.
                     The Otsu threshold, Sobel, Canny and ridge_mask of the reference feed nothing and are not computed.
                     Synchronises `stream`.
   lg_midrib_walk    the ridge walk alone on the host (no device, no handle), over a given enhanced image [H][W] and mask [H][W]
                     (HOST): found = 0 is the reference's None orientation, else orient = angle, major, minor, centre x, centre y
                     (float32, widened to double as Python does).  out[4] / *status as lg_detect_midrib.  The float64 set-up,
                     centre-line and sample arithmetic is the code the device walk runs. */
int lg_clahe(lg_handle h, const uint8_t* src, int B, int H, int W, double clip_limit, int tiles_x, int tiles_y, uint8_t* dst,
             void* stream);
int lg_detect_midrib(lg_handle h, const uint8_t* image, int C, const uint8_t* mask, int B, int H, int W, int32_t* out,
                     int32_t* status, void* stream);
int lg_midrib_walk(const uint8_t* enhanced, const uint8_t* mask, int H, int W, int found, const float* orient, int32_t* out,
                   int32_t* status);

/* ---- training-sample harvesting: EnhancedGraspDataCollector (scripts/utils/ml_grasp_optimizer/data_collector.py)
   lg_harvest_patches   _extract_patches :91-173 (+ the rot90 of _generate_augmented_samples :250-266): raw 32x32 windows
                        [y-16,y+16) x [x-16,x+16) of depth / mask / the seven score planes maps[0..6] of ONE frame around
                        n points xy [n][2] DEVICE, rotated by rot[i] quarter turns (torch.rot90; rot may be NULL).
                        out_depth, out_mask [n][32][32], out_scores [n][7][32][32] f32 DEVICE; flags [n] int32 DEVICE:
                        bit 0 non-finite depth, 1 empty mask patch, 2 non-finite score, 3 window outside the frame:
                        set alone, nothing written for that point.  A window is inside iff 16 <= x <= W-16 and
                        16 <= y <= H-16, where the slices of :103-104 are full -- the far edge is inclusive.  This is
                        NOT _check_boundaries :83-89 (x >= W-16 refused), which collect_sample applies to the
                        positive point only; negatives go straight to _extract_patches.
   lg_negative_masks    the regions negatives are drawn from: tip = (dilate5x5(distance_map) == distance_map) & mask
                        (_get_tip_points :426-443), stem = the mask's bottom quarter eroded twice by the 5x5 ellipse
                        (_get_stem_points :445-460); u8 [H][W] DEVICE each.
   lg_leaf_contour      cv2.findContours(EXTERNAL, CHAIN_APPROX_NONE) + max(contourArea) of _get_edge_points :462-490:
                        every border pixel of the largest outer contour in tracing order, out_xy [cap][2] int32 HOST;
                        *n_out = number of points (may exceed cap: only cap are written). */
int lg_harvest_patches(lg_handle h, const float* depth, const uint8_t* mask, const float* const maps[LG_NUM_MAPS],
                       int H, int W, int n, const int32_t* xy, const int32_t* rot, float* out_depth, float* out_mask,
                       float* out_scores, int32_t* flags, void* stream);
int lg_negative_masks(lg_handle h, const float* distance_map, const uint8_t* mask, int H, int W, uint8_t* out_tip,
                      uint8_t* out_stem, void* stream);
int lg_leaf_contour(lg_handle h, const uint8_t* mask, int H, int W, int32_t* out_xy, int cap, int* n_out, void* stream);

/* Per-kernel device timing with HIP events recorded on the launch stream (bench.py roofline).
   lg_profile_enable(h,1) starts collecting for every kernel (an event pair around each launch);
   lg_profile_enable(h,2) collects only "final", whose dispatch stamps its own start/stop events
   (hipExtLaunchKernelGGL: no extra packets in the stream); 0 stops.  lg_profile_read returns, for kernel `name`
   ("final", "dt_fwd", "dt_bwd", "prep", "stem", "topk", "gather", "cnn", ...), the number of
   launches and their summed duration in milliseconds since the last enable. */
int lg_profile_enable(lg_handle h, int on);
int lg_profile_read(lg_handle h, const char* name, int* launches, double* total_ms);

/* Inspection of the last lg_score_maps / lg_select_grasp call on this handle (synchronises the device):
   out[0], out[1] = max d_in, max d_out of frame `frame` in OpenCV's 16.16 fixed point (the normaliser
   max|d_in - d_out| of calculate_sdf_score, grasp_point_selector.py:531-533, is their maximum / 65536);
   win[0..3] (optional) = the distance-transform sweep window {x0, x1, y0, y1} (half open) used for that frame. */
int lg_debug_dt_max(lg_handle h, int frame, uint32_t out[2], int32_t win[4]);
/* form[0] = 1: d_in of that frame came from the row search (0: from the two sweeps); form[1] = 1: its d_out sweeps were
   skipped (the maximum provably lies on the frame border).  Which form a batch takes is decided on the device. */
int lg_debug_dt_form(lg_handle h, int frame, int32_t form[2]);
/* *algo = the form of the row search the last call queued for its searched frames (LG_DT_SEARCH_ALGO's numbering: 1 one level,
   5 seed pairs + stencil bands, 6 one register sweep per frame; 2 to 4 were the two-level search with recorded minimising rows
   and are no longer taken); 0: the handle queues no search. */
int lg_debug_dt_search_form(lg_handle h, int32_t* algo);
/* The table behind it on the host (no device, no handle): the form a batch of n frames of H x W takes when LG_DT_SEARCH_ALGO is
   `forced` (0: by size).  1 up to 64 x 1080 x 1920 pixels in the batch; above, 6 where 16 <= W <= 2048 and H >= 16, else 5 where
   H, W >= 16, else 1.  Forcing 5 or 6 gives the same answer whatever the batch; forcing 1 gives 1. */
int lg_dt_form_host(int forced, int n, int H, int W);
/* *n = frames of the last lg_score_maps / lg_select_grasp* call that the device orientation kernel handed back (more runs than
   its scratch holds: LG_ORIENT_CAP at lg_create, one cap for the handle's life) and the host threads analysed; 0 where the
   host analyses every frame anyway (LG_HOST_ORIENT at lg_create).
   The small results of a call -- every frame's orientation and status word, the near-tile offsets, the result rows -- are
   written by the kernels straight into the handle's pinned host buffers through their device aliases and read by the host
   behind the events it waits for anyway; LG_DIRECT_HOST=0 at lg_create (or an allocation without an alias): they come back by
   copies on the streams instead.  Same results either way. */
int lg_debug_orient_redo(lg_handle h, int32_t* n);
/* The near tiles of a frame on the host (no device, no handle), the code the device runs: the tiles (64 x 16 pixels) of the
   score-plane kernel whose look at the mask can meet the mask's bounding box [bx0, bx1] x [by0, by1] (bx1 < bx0: empty) in an
   H x W frame, halo = gaussian_size / 2 + 1.  They form a rectangle of the tile grid: rect = {tx_lo, tx_hi, ty_lo, ty_hi},
   inclusive; returns their number, 0 with rect = {0, -1, 0, -1} when there is none, LG_ERR_INVALID for a bad argument.  Every
   other tile is constant whatever the mask.  In sparse mode lg_select_grasp* launches the plane kernel on the near tiles only
   (LG_FINAL_NEAR=0 at lg_create: on every tile, as lg_score_maps does). */
int lg_near_tile_rect(int bx0, int bx1, int by0, int by1, int H, int W, int halo, int32_t rect[4]);
/* The stem words of one frame on the host (no device, no handle), the code the device runs: out[H][WW] = the bit rows of
   dilate(mask & rows [bottom_start, H), ellipse k) & mask for the mask bit rows bits[H][WW] (WW = (W + 63) / 64, bits past W
   zero), 1 <= k <= 64.  The dilation runs as two chains of nested spans from the ellipse's widest row to its end rows: the
   accumulator is dilated by the difference between one row's span and the next narrower one and takes that row; only the words
   of the mask's bounding box, in rows from which the ellipse reaches the bottom region, do arithmetic, every other word is
   written as zero.  LG_STEM_ALGO=0 at lg_create: the device dilates every row's span from scratch instead (the form spans that
   are not nested would take).  Returns 1 (the chains ran), LG_ERR_INVALID for a bad argument.
   lg_stem_words_host_spans: the same for hand-made spans -- n rows, anchor row / column `anchor`, row i covers the columns
   [lo[i], hi[i]] relative to the anchor (lo > hi: empty; entries in [-32, 32], at most 63 columns) -- algo 1: the chains when the
   spans are nested, else the per-row loop; algo 0: the per-row loop.  Returns 1 when the chains ran, 0 for the per-row loop.
   lg_stem_plan: the chains of an ellipse (1 <= k <= 64; n, anchor, lo, hi ignored) or of hand-made spans (k = 0).  Returns 1 when
   the spans are nested (every row non-empty and inside the next row towards the widest one, 0 inside both end rows), else 0;
   *i0 = the widest row, span_lo / span_hi = the spans, dlo[i] / dhi[i] (i != i0) = the ends of the chain's previous row minus
   those of row i (<= 0 / >= 0 when nested).  Output pointers may be null. */
int lg_stem_words_host(const uint64_t* bits, int H, int W, int WW, int bottom_start, int k, uint64_t* out);
int lg_stem_words_host_spans(const uint64_t* bits, int H, int W, int WW, int bottom_start, int n, int anchor, const int8_t* lo,
                             const int8_t* hi, int algo, uint64_t* out);
int lg_stem_plan(int k, int n, int anchor, const int8_t* lo, const int8_t* hi, int32_t* i0, int8_t span_lo[64], int8_t span_hi[64],
                 int8_t dlo[64], int8_t dhi[64]);
/* A frame's sweep window on the host (no device, no handle), the code the device runs.  The bit-row pass reduces a mask to five
   words that all start from zero: box = {max of W - 1 - x, max of x, max of H - 1 - y, max of y, number} over the set pixels
   (the two minima are held as maxima; number 0: empty mask, whatever the other four say).  out = {wx0, wx1, wy0, wy1 (the window:
   columns [wx0, wx1), rows [wy0, wy1)), bx0, bx1, by0, by1 (the bounding box; bx1 < bx0: empty), skip_out (the d_out sweeps have
   nothing to add), search_in (the frame's own eligibility for the row search: search_mode != 0, not empty, at least one zero
   pixel -- a batch may still take the sweeps), area, columns per sweep wave}.  LG_ERR_INVALID for a bad argument or a width
   the sweeps do not take (W > 8192). */
int lg_window_from_box(const uint32_t box[5], int H, int W, int search_mode, int32_t out[12]);
/* Max d_out along one frame border line on the host (no device, no handle), the pruned search the device runs.  prof[i], i in
   [0, n): distance from the line of the nearest leaf pixel in line position lo + i, -1 where there is none; the line has `len`
   positions, 0 <= lo, lo + n <= len, 1 <= n, every entry <= 16384.  *out = max over p in {lo .. lo + n - 1, 0, len - 1} of the
   min over the entries >= 0 of the 5 x 5 chamfer norm of (|p - (lo + i)|, prof[i]) in 16.16 fixed point; 0xFFFFFFFF when no
   entry is >= 0.  LG_ERR_INVALID for a bad argument. */
int lg_border_line_max(const int32_t* prof, int n, int lo, int len, uint32_t* out);
/* off[0 .. B] = first entry of every frame's near tiles in the list the last lg_select_grasp* call on this handle launched its
   plane kernel on (off[0] = 0, off[B] = the list's length; frame b has off[b + 1] - off[b] near tiles).  cap >= B + 1.
   LG_ERR_INVALID when that call did not take the near launch (planes or validity taken back, LG_FINAL_NEAR=0, LG_SUBBATCH,
   LG_NO_SKIP, LG_FINAL_PERSIST / LG_FINAL_TPW, each as the handle found it at lg_create) or cap is too small.  Launches nothing. */
int lg_debug_near_tiles(lg_handle h, int32_t* off, int cap);
/* Tail lanes of lg_select_grasp* ("Tail in lanes"): behind the front, which runs once, the batch is cut into
   lanes of consecutive frames, and every lane runs planes -> top-k -> survivors -> gather -> CNN as a chain on a stream of its
   own, beside the other lanes'.  Results do not depend on the lanes: every row equals the one-lane call's bit for bit.
   lg_tail_lane_plan (host only: no device, no handle) is the rule: B frames, requested = 0 (automatic: LG_TAIL_LANES_AUTO lanes
   from LG_TAIL_LANES_MIN_B frames on, else one) or 1 .. 4 (that many), eligible = the call may run in lanes at all (sparse call
   with the near launch, model loaded, pruned CNN pass, not label-aware, not the candidates entry; 0: one lane).  *sb = frames per
   lane, ceil(B / min(requested lanes, B)); *lanes = ceil(B / *sb), so no lane is empty and only the last may be shorter.
   LG_ERR_INVALID for B < 1, requested outside [0, 4] or a null pointer.
   A call under the automatic rule runs in one lane as well while another handle of the process is inside an lg_select_grasp*
   call (the other batch fills the chip already: two batches in flight measured 5-10 % slower with lanes), and where its
   B * top_k patch slots exceed one slice of the CNN pass (8192): lanes would then hold a slice's worth of activation workspace
   each.  A forced setting ignores both.
   lg_debug_tail_lanes: set = 0 .. 4 stores the request for the handle's later calls, set < 0 only reports; *last (may be null) =
   lanes of the last lg_select_grasp* call on this handle (1 for a call that did not run in lanes; 0 before any, and behind an entry of another family).  Lanes show as
   sub-batches in lg_debug_cnn_survivors.  LG_ERR_INVALID for set > 4. */
int lg_tail_lane_plan(int B, int requested, int eligible, int32_t* lanes, int32_t* sb);
int lg_debug_tail_lanes(lg_handle h, int set, int32_t* last);
/* The experiment switches as text, one "NAME=value\n" line per switch ("Experiment switches", has the rows).
   lg_options_text (host only: no device, no handle): the environment as it is now, through the parser of `which` -- 0 a
   handle's switches (lg_create), 1 a model's (lg_cnn_load*), 2 a trainer's (lg_train_create).  lg_debug_options: the values the
   handle stored at lg_create, which hold for its life.  A presence-only switch prints 0 / 1, an unset LG_FINAL_PERSIST /
   LG_FINAL_TPW -1, LG_CNN_DIRECT shows as LG_CNN_WINO_MASK=0 and LOCAL_WORLD_SIZE in LG_HOST_THREADS.  buf[cap] takes the text,
   cut to fit and always terminated; returns the length of the whole text, LG_ERR_INVALID for a bad argument. */
int lg_options_text(int which, char* buf, int cap);
int lg_debug_options(lg_handle h, char* buf, int cap);
/* *patches = how many patches the last lg_select_grasp* call on this handle put through the CNN (0 without a model;
   B * top_k where every candidate is scored: lg_select_grasp_candidates*, LG_CNN_PRUNE=0).  Synchronises the device. */
int lg_debug_cnn_scored(lg_handle h, int64_t* patches);
/* The clutter arg-max of the last lg_leaf_stats / lg_leaf_stats_batch / lg_leaf_select_batch call on this handle: *n_frames =
   its batch size (0: no such call yet, or the call was refused before the pass), flags[b] = 1 for a frame whose survivor
   list of the branch-and-bound pass overflowed, *n_flagged = how many did.  *n_flagged > 0 means the full-transform pass
   (column scan + per-row lower envelope) ran for the whole batch and every frame's arg-max comes from it.  flags: HOST, cap
   >= the batch size (LG_ERR_INVALID otherwise).  Read-only, launches nothing. */
int lg_debug_leaf_fallback(lg_handle h, int32_t* flags, int cap, int32_t* n_frames, int32_t* n_flagged);
/* The CNN pass of the last lg_select_grasp* call on this handle, patch by patch.  The call's B frames run as *n_sub
   sub-batches of *sub_frames frames (one sub-batch of B frames unless LG_SUBBATCH was set at lg_create); sub-batch k owns
   the entries [k * *sub_frames * top_k, ...) of list, slot and logits, one per candidate slot of its frames, and every index
   below counts from the sub-batch's first entry:
     counts[k]   patches of sub-batch k that went through the CNN (counts_cap >= *n_sub entries);
     list[j]     j < counts[k]: frame * top_k + candidate of patch j (frame-major, candidates ascending); -1 past the count;
     slot[i]     candidate slot i = frame * top_k + candidate -> its patch, -1: pruned (no patch, no logit);
     logits[j]   the logit of patch j; entries past the count are whatever the buffer held before the call.
   *n_slots = B * top_k, the entries written to each of list, slot and logits (cap >= *n_slots entries each).  Where every
   candidate is scored (lg_select_grasp_candidates*, LG_CNN_PRUNE=0) this is the identity: counts[k] = its frames * top_k,
   list[j] = slot[j] = j.  Synchronises the device and launches nothing.  Size query: counts, list, slot and logits all NULL
   with counts_cap = cap = 0 sets *sub_frames, *n_sub and *n_slots, copies nothing and returns LG_OK.  LG_ERR_INVALID: any
   other NULL pointer, arrays too small, or no such call with a model loaded since the workspace was last (re)allocated;
   LG_ERR_BUSY: a call in flight. */
int lg_debug_cnn_survivors(lg_handle h, int32_t* sub_frames, int32_t* n_sub, int32_t* counts, int32_t counts_cap,
                           int32_t* list, int32_t* slot, float* logits, int64_t cap, int64_t* n_slots);
/* Deferred planes.  A call that takes no plane and no validity back (sparse mode) does not store five of the feature planes
   (sdf, approach, isolation, accessibility, stem): its plane kernel stores what top-k reads and flatness, and the patch gather
   computes those five itself at the pixels of its 32 x 32 windows, with the plane kernel's per-pixel code -- the patches are the
   same floats.  LG_DEFER_PLANES=0 at lg_create: such calls store and read the planes as calls that take planes back do.
   lg_debug_patch: out[9][32][32] = the patch in slot `slot` of the last lg_select_grasp* call with a model loaded, as the CNN
   read it (slot: an entry of lg_debug_cnn_survivors' list, counted from the start of the buffer: sub-batch k's slots start at
   k * sub_frames * top_k).  LG_ERR_INVALID past the slots of that call.  Synchronises the device, launches nothing.
   lg_debug_ws_plane_bytes: bytes[i] = device memory the handle holds for its own copy of plane i (0: never needed; a handle
   that has only made sparse calls holds distance, traditional and flatness only).
   lg_wave_rows_on_mask (no device, no handle; the code the gather runs): 1 when any mask bit is set in word w of the rows
   (y & ~3) .. (y & ~3) + 3 below H of the bit rows bits[H][WW] -- the rows and columns one wave of the plane kernel covers: where
   it is 0 that wave stored +0.0 in every masked plane, where it is 1 a pixel off the mask got (expression) * 0, which can be
   -0.0.  0 otherwise, LG_ERR_INVALID for a bad argument. */
int lg_debug_patch(lg_handle h, int64_t slot, float* out);
/* lg_debug_isolation_fields: the two raw 16.16 chamfer-3 transforms of frame `frame` of the last lg_select_grasp*_labels call
   with label_aware = 1 on this handle: dc_fix / dw_fix [H][W] HOST (either may be NULL), the transforms of 1 - ic and 1 - iw
   over the WHOLE frame (the two raster sweeps compute every pixel), max_fix[2] their whole-frame maxima.  Returns 1 when the
   frame had another leaf and the fields were computed, 0 when it took the closed form (nothing is written), < 0 on error (no
   such call, or a later call reused the workspace). */
int lg_debug_isolation_fields(lg_handle h, int frame, uint32_t* dc_fix, uint32_t* dw_fix, uint32_t max_fix[2]);
/* Host forms of the label-aware arithmetic (no device, no handle).
   lg_norm3_host: out[i] = N3(|dx[i]|, |dy[i]|) = (max - min) * 62587 + min * 89738, the closed-form norm of the (0.955, 1.3693)
   chamfer mask in 16.16: on a frame with a zero pixel the two raster passes give min over the zero pixels q of N3(p - q).
   lg_dilate_words_host: out = cv2.dilate(bits, ellipse k) on bit rows [H][WW] (bit j of word w = pixel 64 w + j; bits past W
   are ignored and come out 0), 1 <= k <= 64 -- the per-word code of the device's whole-frame dilation. */
/* lg_label_aware_check: the rule every entry applies to lg_params.label_aware -- LG_OK for 0, and for 1 when the entry has a
   label image (has_labels != 0: lg_select_grasp_labels, lg_select_grasp_candidates_labels); LG_ERR_INVALID for 1 on an entry
   that takes a mask (lg_select_grasp, lg_select_grasp_candidates, lg_score_maps) and for any other value. */
int lg_label_aware_check(const lg_params* p, int has_labels);
int lg_norm3_host(const int32_t* dx, const int32_t* dy, int n, uint32_t* out);
int lg_dilate_words_host(const uint64_t* bits, int H, int W, int WW, int k, uint64_t* out);
int lg_debug_ws_plane_bytes(lg_handle h, int64_t bytes[LG_NUM_MAPS]);
int lg_wave_rows_on_mask(const uint64_t* bits, int H, int WW, int y, int w);

/* ---- GraspPointCNN training step: one call = one iteration of the inner loop of
   scripts/train_model.py:247-265 (zero_grad, forward in train mode, BCEWithLogitsLoss(pos_weight), backward,
   clip_grad_norm_(max_grad_norm), Adam step with L2 weight_decay) on the model of
   scripts/utils/ml_grasp_optimizer/model.py:5-128 with any LG_ATT_* attention (LG_ATT_SPATIAL = the script's model).
   Flat parameter vector = model.parameters() order; flat buffer vector = running_mean, running_var of every BatchNorm
   in module order.  Dropout keep masks: one [N][width] block per dropout layer, concatenated in module order
   (Dropout2d of every encoder block: width = filters[b]; classifier Dropout 0.5 / 0.5 / 0.4: widths F, F/2, F/4),
   values 0 or 1/(1-p); NULL = drawn on the device from `seed` and the step counter. */
typedef struct lg_trainer lg_trainer;
typedef struct lg_train_hparams {
    float lr, beta1, beta2, eps, weight_decay;   /* train_model.py:222: Adam(lr=0.0005, weight_decay=0.01), betas (0.9, 0.999), eps 1e-8 */
    float max_grad_norm;                         /* :256 clip_grad_norm_(max_norm=1.0); <= 0: no clipping */
    float pos_weight;                            /* :221 BCEWithLogitsLoss(pos_weight=2.0) */
} lg_train_hparams;
int lg_train_create(int device, int n_blocks, const int32_t* filters, int attention_type, int max_batch, lg_trainer** out);
int lg_train_destroy(lg_trainer* t);
const char* lg_train_last_error(lg_trainer* t);
int lg_train_sizes(lg_trainer* t, int64_t* n_params, int64_t* n_buffers, int64_t* mask_row);
/* HOST arrays; exp_avg / exp_avg_sq may be NULL (= zeros: a fresh optimizer) */
int lg_train_set_state(lg_trainer* t, const float* params, const float* buffers, const float* exp_avg,
                       const float* exp_avg_sq, int64_t step);
/* HOST arrays, any may be NULL; grads = the unclipped gradients of the last step */
int lg_train_get_state(lg_trainer* t, float* params, float* buffers, float* exp_avg, float* exp_avg_sq, float* grads,
                       int64_t* step);
/* x [N][9][32][32], labels [N], masks (or NULL), logits_dev (or NULL): DEVICE pointers.  apply_update = 0: loss and
   gradients only (BatchNorm running statistics still move, as in a train-mode forward).  loss_host / grad_norm_host
   (or NULL) make the call synchronous. */
int lg_train_step(lg_trainer* t, const float* x, const float* labels, int N, const float* masks, uint64_t seed,
                  const lg_train_hparams* hp, int apply_update, float* loss_host, float* grad_norm_host, float* logits_dev);
int lg_train_sync(lg_trainer* t);
/* lg_train_epoch: the steps of one epoch in one call, nothing between them on the host -- it leaves every float where the
   same sequence of lg_train_step(masks = NULL, apply_update = 1) calls leaves it.
     x [n][9][32][32], labels [n]   DEVICE, 16-byte aligned x: the whole training set; it stays where it is.
     idx [m]                        HOST: sample numbers in drawing order (what WeightedRandomSampler / torch.multinomial
                                    returns).  Every entry is checked against [0, n) before anything is enqueued.
   Step k takes idx[k * batch .. min(m, (k + 1) * batch)) in that order; a last step of fewer than 2 samples is skipped
   (BatchNorm in train mode), m < 2 runs no step: lg_train_epoch_plan states the rule on the host (number of steps, size of
   the last one run, 0 when there is none), without a device or a trainer; LG_ERR_INVALID for batch < 2 or m outside
   [0, INT32_MAX].  Per step, on the trainer's stream: a gather kernel writes the step's rows straight into the step's input
   buffers (in place of lg_train_step's device-to-device copies), the step runs with dropout masks drawn on the device from
   `seed` and the device's step counter, and a one-workgroup kernel files loss and gradient norm into device slot k, adds
   the step's correct predictions to a device counter and copies its logits to logits_dev + k * batch.  idx, hp and seed
   are uploaded once; one copy-back and one stream synchronisation end the call.
     losses, grad_norms             HOST, capacity lg_train_epoch_plan's n_steps
     correct                        HOST: predictions with (logit > 0) == (label == 1).  trainer.py's fit() writes
                                    sigmoid(logit) > 0.5 in float32; the two differ only for 0 < logit <~ 1.2e-7, where
                                    the float32 sigmoid rounds to exactly 0.5
     logits_dev                     DEVICE [m]; the entries of a skipped tail are not written
     n_steps                        HOST: steps run.  Any of these five may be NULL.
   LG_ERR_INVALID, with the trainer untouched: an index outside [0, n), batch outside [2, max_batch], a NULL t / x / labels /
   hp, a NULL idx with m > 0, n or m above INT32_MAX, x not 16-byte aligned.
   LG_TRAIN_STREAMS=2 is honoured (the step's last act is to wait for its side stream, so consecutive steps cannot overlap
   on the shared buffers).  LG_TRAIN_GRAPH=1 is not: the epoch always issues plain launches, because a captured step
   replayed back to back without a host synchronisation in between has never been run, and the memset node that step once
   replayed wrongly (see zero_grads in lg_train.hip) is reason enough not to start here.
   A HIP error in the middle returns its code; the weights are then whatever the completed steps left, and the step count
   lg_train_get_state reports counts the steps enqueued up to there. */
int lg_train_epoch(lg_trainer* t, const float* x, const float* labels, int64_t n, const int32_t* idx, int64_t m, int batch,
                   uint64_t seed, const lg_train_hparams* hp, float* losses, float* grad_norms, int64_t* correct,
                   float* logits_dev, int32_t* n_steps);
int lg_train_epoch_plan(int64_t m, int batch, int32_t* n_steps, int32_t* last_n);
/* Data-parallel training (one process per GPU): lg_train_step(apply_update = 0) on the rank's shard of the batch, average
   the flat gradient vector over the ranks (RCCL all-reduce on a tensor wrapping *dev_ptr; lg_train_sync first), then
   lg_train_apply = clip_grad_norm_ + Adam.step() on the averaged gradients (train_model.py:256-258).  BatchNorm statistics
   stay per rank, as with torch's DistributedDataParallel without SyncBatchNorm. */
int lg_train_grad_buffer(lg_trainer* t, float** dev_ptr, int64_t* n);
int lg_train_apply(lg_trainer* t, const lg_train_hparams* hp, float* grad_norm_host);

/* ---- trainer -> inference hand-off and validation on the device (scripts/train_model.py:280-311)
   lg_cnn_load_from_trainer   lg_cnn_load without the host: the one fold both entries share (device kernels: BatchNorm
                     folding, the direct, F(2x2) and F(4x4) Winograd weight layouts, the transposed classifier; IEEE double
                     operations in a fixed order, rounded once) reads the trainer's flat parameter and buffer vectors where
                     lg_cnn_load reads a device copy of the caller's host tensors, so every float equals what lg_cnn_load
                     writes for trainer.state_dict.  Whether the inference kernels take the model is decided
                     before anything is touched -- lg_cnn_load's conditions and messages, and the classifier sizes a forward
                     would refuse: on LG_ERR_UNSUPPORTED / LG_ERR_INVALID (a null trainer, a trainer on another device) the
                     model loaded before stays loaded and usable.  Same geometry as the loaded model (encoder_filters,
                     attention_type): the weight buffers are rewritten in place, nothing is freed or allocated and the
                     activation workspace stays; otherwise as lg_cnn_load (which always frees first and allocates anew).
                     LG_CNN_F23 / LG_CNN_DIRECT / LG_CNN_WINO_MASK are read at the end of either load.
                     Ordering: the fold runs on the legacy default stream behind an event recorded on the trainer's own
                     stream(s) -- no lg_train_sync is needed after lg_train_step -- and that stream is synchronised before
                     the call returns: a forward enqueued on any stream afterwards reads the new weights.  A forward still
                     in flight on a NON-BLOCKING stream is the caller's to synchronise first (blocking streams, torch's
                     default stream among them, are ordered by the legacy default stream itself).
   lg_eval_logits    validation loss and confusion counts of N labelled logits (DEVICE, float32), walked in chunks of
                     `chunk` samples as DataLoader(batch_size=chunk, shuffle=False) would (:280-298): chunk c covers
                     [c chunk, min(N, (c + 1) chunk)).  Per sample, in double from the float logit z and label y:
                     (1 - y) z + (1 + (pos_weight - 1) y) (max(-z, 0) + log1p(exp(-|z|))), BCEWithLogitsLoss(pos_weight).
                     A chunk's mean = its terms added in index order / its length; loss = the chunk means added in chunk
                     order / n_chunks (:306).  The order is fixed (it does not depend on the grid; no float atomics): two
                     calls give the same bits.  Counts as analyze_predictions (:64-99): pred = z > threshold compared in
                     float (the reference thresholds the LOGIT), tp = pred & y == 1, tn = !pred & y == 0, fp = #(y == 0) -
                     tn, fn = #(y == 1) - tp.  correct counts (z > 0) == (y == 1): the reference's sigmoid(z) > 0.5 (:285-287)
                     everywhere except for 0 < z < ~6e-8, where the float sigmoid rounds to exactly 0.5 and the reference
                     predicts 0.  A NaN logit follows IEEE: not predicted positive, loss NaN.  N < 1, chunk < 1 or a null
                     pointer: LG_ERR_INVALID.  Synchronises `stream`; the result is a HOST struct.
   lg_eval_logits_host   the same code on the host (logits, labels HOST; no device, no handle): the per-sample term and the
                     chunk walk are shared with the kernels; device and host differ in the ulps of exp / log1p only.
   lg_cnn_evaluate   lg_cnn_forward on patches [N][9][32][32] (same plan, same slices: the same logits bit for bit), then
                     lg_eval_logits on them, on one stream.  labels [N] DEVICE; logits_out: DEVICE, N floats, or NULL.
                     Synchronises `stream`.
   lg_debug_cnn_weights   plain read-back of one weight buffer of the loaded model into out (HOST, cap floats): which =
                     LG_CNNW_*, layer = encoder layer (BCONV .. UWINO4) or classifier layer (FCW, FCB), ignored otherwise.
                     *n = its floats, 0 when the model has no such buffer (WCONV past layer 0 of a non-standard encoder,
                     UWINO of layer 0, attention tensors of another attention type).  cap = 0: size query.  LG_CNNW_SCALARS:
                     n_layers, F, Fp, npix, act_per_patch, standard, att_type, att_b (0 without spatial attention), then
                     cin, cout, cinp, coutp, wi, pool of every layer, as floats.  LG_CNNW_ALLOCS: copies nothing; *n = the
                     weight buffers lg_cnn_load and lg_cnn_load_from_trainer have allocated on this handle so far (an
                     in-place refresh adds none: the buffers sit where they sat).  Synchronises the device. */
enum { LG_CNNW_BCONV = 0, LG_CNNW_WCONV = 1, LG_CNNW_UWINO = 2, LG_CNNW_UWINO4 = 3, LG_CNNW_FCW = 4, LG_CNNW_FCB = 5,
       LG_CNNW_ATT_W = 6, LG_CNNW_CA_W1 = 7, LG_CNNW_CA_B1 = 8, LG_CNNW_CA_W2 = 9, LG_CNNW_CA_B2 = 10, LG_CNNW_ZEROS = 11,
       LG_CNNW_SCALARS = 12, LG_CNNW_ALLOCS = 13 };
typedef struct lg_eval_result {      /* HOST, 64 bytes */
    double  loss;                    /* mean over the chunks of each chunk's mean      train_model.py:280-298 */
    int64_t n, n_chunks;
    int64_t correct;                 /* (logit > 0) == (label == 1)                     :285-287 */
    int64_t tp, fp, fn, tn;          /* analyze_predictions, threshold on the LOGIT     :64-99 */
} lg_eval_result;
int lg_cnn_load_from_trainer(lg_handle h, lg_trainer* t);
int lg_eval_logits(lg_handle h, const float* logits, const float* labels, int N, int chunk, double pos_weight, float threshold,
                   lg_eval_result* out, void* stream);
int lg_eval_logits_host(const float* logits, const float* labels, int N, int chunk, double pos_weight, float threshold,
                        lg_eval_result* out);
int lg_cnn_evaluate(lg_handle h, const float* patches, const float* labels, int N, int chunk, double pos_weight, float threshold,
                    float* logits_out, lg_eval_result* out, void* stream);
int lg_debug_cnn_weights(lg_handle h, int which, int layer, float* out, int64_t cap, int64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* LEAFGRASP_H */
