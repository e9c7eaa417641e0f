// Experiment and sizing switches of liblgrasp.so.  lg_options.cpp is the only place that reads the environment: one struct per
// object that is configured, one field here and one line there per switch ("Experiment switches": the same rows).
#pragma once

// list entries per workgroup of the near launch (lg_launch_final; LG_FINAL_NEAR=n overrides).  256 frames of 1080p, plane kernel
// alone: 1 / 2 / 4 / 8 entries 0.275 / 0.273 / 0.305 / 0.328 ms (profiles/NOTES_near_tiles.md).  The launch applies at every batch
// size: the enumeration kernel (then in front of the orientation kernel, with a copy) did not lengthen a call of 1 or 32 frames.
#ifndef LG_FINAL_NEAR_TPW
#define LG_FINAL_NEAR_TPW 1
#endif

struct LgOptions {   // a handle's: read ONCE, by lg_create (never on the per-call path), kept for its life (lg_debug_options)
    int host_threads = 8;        // LG_HOST_THREADS=n; unset: this process's share of the CPUs it may run on (one process per GPU:
                                 //            LOCAL_WORLD_SIZE ranks split the node), at most 16
    int subbatch = 0;            // LG_SUBBATCH=n: sub-batch multi-stream pipeline inside lg_select_grasp (0 = off)
    bool trace = false;          // LG_TRACE: per-call timeline on stderr
    int no_skip = 0;             // LG_NO_SKIP=1: lg_final_kernel without the constant-tile fast path (dense-path roofline);
                                 //            =3: also without the wave-level off-leaf shortcut (both bits leave the results unchanged)
    int final_near = LG_FINAL_NEAR_TPW;   // LG_FINAL_NEAR=0: lg_final_kernel walks every tile in sparse mode too (the launch before the
                                 //            near launch; A/B, tests); =n: near launch with n list entries per workgroup
    int final_persist = -1;      // LG_FINAL_PERSIST=n: n resident workgroups per CU walk the tiles; LG_FINAL_TPW=n: n consecutive tiles per
    int final_tpw = -1;          //            workgroup (lg_launch_final; < 0: the mode's default).  Either one set: final_near = 0
    bool host_orient = false;    // LG_HOST_ORIENT: contour analysis of every frame on the host threads (the round-1 path)
    bool cnn_prune = true;       // LG_CNN_PRUNE=0: every candidate's patch goes through the CNN (A/B, tests)
    bool defer_planes = true;    // LG_DEFER_PLANES=0: sparse calls store and read all six feature planes, as before the deferred mode (A/B, tests)
    int dt_search = 2;           // LG_DT_SEARCH=0: d_in by the two sweeps for every frame; 1: by the row search wherever it applies;
                                 // 2 (default): per frame, the search while the batch's estimated search work stays below the sweeps' latency
    int dt_algo = 0;             // LG_DT_SEARCH_ALGO=1: one-level row search at every batch size; 5: seed row pairs + stencil bands;
                                 // 6: one two-wave register sweep per frame; 0: by batch size (lg_dt_form, lg_dt.h)
    int dt_band_p = 16, dt_band_e = 4;   // LG_DT_BAND_P=12 | 16 | 24 | 32: rows from one seed pair of form 5 to the next;
                                 // LG_DT_BAND_E=2 | 4: columns per lane of its band kernel (experiments, tests)
    int side_tail = 1;           // LG_SIDE_TAIL=0: frame-border maxima + stem bits after the sweeps on the caller's stream (round 1); 1: on the
                                 // side stream behind the orientation kernel; 2: on a third stream
    bool stem_algo = true;       // LG_STEM_ALGO=0: stem bits by the per-row kernel (A/B, tests); 1: two chains of nested spans
    bool direct_host = true;     // LG_DIRECT_HOST=0: the small results come back by hipMemcpyAsync (A/B, tests)
    int orient_cap = 16384;      // LG_ORIENT_CAP=n: runs per frame held by the orientation scratch, the midrib scratch's too (tests lower it
                                 // to reach the host hand-off)
    bool orient_fail = false;    // LG_ORIENT_FAIL: the orientation scratch's set-up fails (the test of the hand-over to the host analysis)
};
struct LgCnnOptions {   // a model's (standard encoder): read once per load, so one handle can reload under other values
    bool f23 = false;            // LG_CNN_F23: the F(2x2,3x3) Winograd kernels instead of F(4x4,3x3)
    int wino_mask = 0x3f;        // LG_CNN_WINO_MASK=<bits>: bit L = layer L on Winograd; LG_CNN_DIRECT: 0, direct implicit GEMM for every layer
};
struct LgTrainOptions {   // a trainer's: read once per lg_train_create
    bool graph = false;          // LG_TRAIN_GRAPH=1: replay the step as a captured graph (measured: no gain)
    int streams = 1;             // LG_TRAIN_STREAMS=2: backward-weights on a second stream; 1: in line
    int conv_small_below = 256, conv_split_below = 256;   // LG_TRAIN_CONV_SMALL / LG_TRAIN_CONV_SPLIT: convolution shape thresholds (lgt_conv)
};
LgOptions lg_options_from_env();
LgCnnOptions lg_cnn_options_from_env();
LgTrainOptions lg_train_options_from_env();
// "NAME=value\n" per switch into buf[cap], cut to fit and terminated; returns the whole length (lg_debug_options; lg_options_text)
int lg_options_print(const LgOptions& o, char* buf, int cap);
