// The tail of select_grasp_point on the device: CNN rescoring, 3-D and pre-grasp point of the pick, and every candidate ranked.
// Reference semantics: scripts/utils/grasp_point_selector.py (cited per kernel); design: DESIGN.md.
#include "lg_finish.h"

// ============================================================================ the tail of select_grasp_point, per frame
// grasp_point_selector.py:205-245 after the candidates exist: CNN rescoring (ml = tanh(3 sigmoid(logit)) / 2 + 1/2, confidence
// weights, "take it if the combined score beats the best so far", :210-237), get_3d_grasp_point (:152-180) and
// calculate_pre_grasp_point (:754-819: five probes of the leaf mask dilated by the clearance ellipse along the viewing ray,
// fallback at 0.10 m).  One wave per frame; the same float64 operations in the same order as the host code this replaces (fp
// contraction off), the selection loop sequential in lane 0 -- the call no longer ships candidate lists, logits and bit rows to
// the host and walks the frames there (0.1 ms of host work + five copies per 256-frame call, with the GPU idle behind them).
// CNN rescoring of candidate i of frame b (:210-237): ml = get_ml_score's tanh(3 sigmoid(logit)) / 2 + 1/2 (:133-136), its
// confidence (:222), weight (:223) and combined score (:226).  false: a border candidate of a torch.bool mask has no ML score
// (SURVEY App. B.7).  lg_finish_kernel and lg_candidates_kernel both call this.
__device__ inline bool lg_ml_rescore(const LgFinishArgs& a, int b, int i, int x, int y, double trad, double* ml_out,
                                     double* conf_out, double* comb_out) {
#pragma clang fp contract(off)
    if (a.mask_is_bool && (x < 16 || y < 16 || x + 16 > a.W || y + 16 > a.H)) return false;
    // (a.slot: the CNN ran on the survivors only; a candidate that cannot beat candidate 0 has no patch and is never taken)
    int j = b * a.K + i;
    if (a.slot) {
        j = a.slot[j];
        if (j < 0) return false;
        j += (b / a.slot_frames) * a.slot_frames * a.K;
    }
    lg_ml_combine((double)a.logits[j], trad, ml_out, conf_out, comb_out);
    return true;
}

struct LgPoint3d { float X, Y, Z; int has_pre; float pX, pY, pZ; };

// get_3d_grasp_point (:152-180) of pixel (x, y) at depth Z and calculate_pre_grasp_point (:754-819): five probes of the leaf
// mask dilated by the clearance ellipse along the viewing ray, fallback at 0.10 m.  Called by every lane of ONE wave with the
// same arguments (lane i tests row i of the structuring element; __ballot): every lane gets the same result.
__device__ inline LgPoint3d lg_point_3d_pre(const LgFinishArgs& a, int b, int x, int y, double Z, int lane) {
#pragma clang fp contract(off)
    const int H = a.H, W = a.W, WW = a.WW;
    LgPoint3d R;
    R.has_pre = 0; R.pX = 0.f; R.pY = 0.f; R.pZ = 0.f;
    const double X = Z * ((double)x - a.cx) / a.f;
    const double Y = Z * ((double)y - a.cy) / a.f;
    R.X = (float)X; R.Y = (float)Y; R.Z = (float)Z;
    const double nrm = sqrt(X * X + Y * Y + Z * Z);
    if (!(nrm > 0.0) || !isfinite(nrm)) return R;    // reference: exception -> None
    const double dxn = X / nrm, dyn = Y / nrm;
    const unsigned long long* fb = a.bits + (size_t)b * H * WW;
    const unsigned long long* fb2 = a.bits2 ? a.bits2 + (size_t)b * H * WW : nullptr;   // label-aware mode: the other leaves
    bool done = false;
    for (int step = 0; step < 5 && !done; step++) {
        // np.arange(0.05, 0.10, 0.01)[step] = start + step * ((start + delta) - start)
        const double dist = 0.05 + (double)step * ((0.05 + 0.01) - 0.05);
        const double tx = X - dxn * dist, ty = Y - dyn * dist, tz = Z;
        const int u = (int)((tx * a.f / tz) + a.cx);
        const int v = (int)((ty * a.f / tz) + a.cy);
        if (!(u >= 0 && u < W && v >= 0 && v < H)) continue;
        // dilated[v, u] != 0  <=>  some set pixel under the ellipse centred there: lane i tests row i of the structuring element
        bool hit = false;
        if (lane < a.se.n && a.se.lo[lane] <= a.se.hi[lane]) {
            const int yy = v + lane - a.se.anchor;
            const int x0 = max(u + a.se.lo[lane], 0), x1 = min(u + a.se.hi[lane], W - 1);
            if (yy >= 0 && yy < H && x0 <= x1) {
                const unsigned long long* row = fb + (size_t)yy * WW;
                for (int w = x0 >> 6; w <= (x1 >> 6); w++) {
                    unsigned long long m = ~0ull;
                    if (w == (x0 >> 6)) m &= ~0ull << (x0 & 63);
                    if (w == (x1 >> 6)) m &= ~0ull >> (63 - (x1 & 63));
                    hit |= (row[w] & m) != 0ull;
                    if (fb2) hit |= (fb2[(size_t)yy * WW + w] & m) != 0ull;
                }
            }
        }
        if (__ballot(hit) == 0ull) {
            const double dg = sqrt((tx - X) * (tx - X) + (ty - Y) * (ty - Y));
            if (dg >= 0.05) { R.pX = (float)tx; R.pY = (float)ty; R.pZ = (float)tz; done = true; }
        }
    }
    if (!done) { R.pX = (float)(X - dxn * 0.10); R.pY = (float)(Y - dyn * 0.10); R.pZ = (float)Z; }
    R.has_pre = 1;
    return R;
}

__global__ __launch_bounds__(64) void lg_finish_kernel(LgFinishArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_comb[64];
    __shared__ int s_elig[64], s_best, s_ml;
    __shared__ double s_bs;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.cand_n[b], K = a.K;
    lg_grasp_result R;
    R.found = 0; R.x = 0; R.y = 0; R.X = 0.f; R.Y = 0.f; R.Z = 0.f; R.has_pre = 0; R.pX = 0.f; R.pY = 0.f; R.pZ = 0.f;
    R.n_candidates = n; R.ml_used = 0; R.best_score = 0.f; R.theta = a.fp[b].theta;
    if (n <= 0) {   // reference: "No valid candidate points found" -> (None, None, None)
        if (lane == 0) a.out[b] = R;
        return;
    }
    const int32_t* xy = a.cand_xy + (size_t)b * K * 2;
    const float* info = a.cand_info + (size_t)b * K * 2;
    const bool rescoring = a.use_cnn && n > 1;
    double comb = 0.0, ml, conf;
    int elig = 0;
    if (rescoring && lane < n)
        elig = lg_ml_rescore(a, b, lane, xy[2 * lane], xy[2 * lane + 1], (double)info[2 * lane], &ml, &conf, &comb) ? 1 : 0;
    s_comb[lane] = comb;
    s_elig[lane] = elig;
    __syncthreads();
    if (lane == 0) {
        int best = 0, ml_used = 0;
        double best_score = (double)info[0];  // candidate 0's traditional score (:205-206)
        if (rescoring)
            for (int i = 0; i < n; i++)
                if (s_elig[i] && s_comb[i] > best_score) { best_score = s_comb[i]; best = i; ml_used = 1; }
        s_best = best; s_ml = ml_used; s_bs = best_score;
    }
    __syncthreads();
    const int best = s_best;
    R.found = 1;
    R.ml_used = s_ml;
    R.x = xy[2 * best]; R.y = xy[2 * best + 1];
    R.best_score = (float)s_bs;
    const LgPoint3d g = lg_point_3d_pre(a, b, R.x, R.y, (double)info[2 * best + 1], lane);
    R.X = g.X; R.Y = g.Y; R.Z = g.Z;
    R.has_pre = g.has_pre; R.pX = g.pX; R.pY = g.pY; R.pZ = g.pZ;
    if (lane == 0) a.out[b] = R;
}

void lg_launch_finish(const LgFinishArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lg_finish_kernel, dim3(a.B), dim3(64), 0, s, a);
}

// ============================================================================ every candidate, ranked
// One workgroup per frame.  Lanes compute each candidate's ML fields (lg_ml_rescore: the operations lg_finish_kernel runs);
// then lane 0 of wave 0 ranks them (lg_rank_candidates, the host export's code) while waves 1.. compute each candidate's 3-D
// and pre-grasp point, one wave per candidate (lg_point_3d_pre; the point does not depend on the rank, so the two overlap);
// then the rows are written in rank order from LDS.  Rows past n get index -1 and zeros.  Rank 0 is lg_finish_kernel's row.
// (Measured: four waves that each took the ranks wave, wave + 4, ... after the ranking: 0.053 ms per launch at any B.)
#define LG_CAND_WAVES 16
__global__ __launch_bounds__(64 * LG_CAND_WAVES) void lg_candidates_kernel(LgFinishArgs a, lg_grasp_candidate* __restrict__ rows) {
#pragma clang fp contract(off)
    __shared__ double s_trad[64], s_comb[64], s_ml[64], s_conf[64], s_pick[64];
    __shared__ int32_t s_scored[64], s_order[64], s_by[64];
    __shared__ LgPoint3d s_pt[64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int K = a.K, n = min(a.cand_n[b], K);
    const int32_t* xy = a.cand_xy + (size_t)b * K * 2;
    const float* info = a.cand_info + (size_t)b * K * 2;
    const bool rescoring = a.use_cnn && n > 1;
    if (t < n) {
        const double tr = (double)info[2 * t];
        double ml = __builtin_nan(""), conf = __builtin_nan(""), comb = __builtin_nan("");
        const bool sc = rescoring && lg_ml_rescore(a, b, t, xy[2 * t], xy[2 * t + 1], tr, &ml, &conf, &comb);
        s_trad[t] = tr; s_comb[t] = comb; s_ml[t] = ml; s_conf[t] = conf;
        s_scored[t] = sc ? 1 : 0;
    }
    __syncthreads();
    if (wave == 0) {
        if (lane == 0) lg_rank_candidates(s_trad, s_comb, s_scored, n, rescoring ? 1 : 0, s_order, s_pick, s_by);
    } else {
        for (int i = wave - 1; i < n; i += LG_CAND_WAVES - 1) {   // wave-uniform: lg_point_3d_pre ballots across the wave
            const LgPoint3d g = lg_point_3d_pre(a, b, xy[2 * i], xy[2 * i + 1], (double)info[2 * i + 1], lane);
            if (lane == 0) s_pt[i] = g;
        }
    }
    __syncthreads();
    lg_grasp_candidate* out = rows + (size_t)b * K;
    for (int r = t; r < K; r += 64 * LG_CAND_WAVES) {
        lg_grasp_candidate R;
        memset(&R, 0, sizeof(R));
        R.index = -1;
        if (r < n) {
            const int i = s_order[r];
            R.index = i;
            R.x = xy[2 * i]; R.y = xy[2 * i + 1];
            R.traditional = info[2 * i];
            R.ml_score = (float)s_ml[i]; R.ml_confidence = (float)s_conf[i]; R.combined = (float)s_comb[i];
            R.scored = s_scored[i];
            R.pick_score = (float)s_pick[r];
            R.by_ml = s_by[r];
            const LgPoint3d g = s_pt[i];
            R.X = g.X; R.Y = g.Y; R.Z = g.Z;
            R.has_pre = g.has_pre; R.pX = g.pX; R.pY = g.pY; R.pZ = g.pZ;
        }
        out[r] = R;
    }
}

void lg_launch_candidates(const LgFinishArgs& a, lg_grasp_candidate* rows, hipStream_t s) {
    hipLaunchKernelGGL(lg_candidates_kernel, dim3(a.B), dim3(64 * LG_CAND_WAVES), 0, s, a, rows);
}
