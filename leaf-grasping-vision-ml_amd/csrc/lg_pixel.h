// Per-pixel device code that the plane kernel (lg_planes.hip), the deferred gather (lg_patches.hip) and top-k (lg_topk.hip)
// share bit for bit: the orderable score key, the constant tile's flatness, and the per-pixel arithmetic of the score planes.
// Device code only (gfx950).
#pragma once
#include "lg_internal.h"

__device__ __forceinline__ uint32_t lg_orderable(float s) {  // monotone float -> uint32 map
    if (s == 0.0f) s = 0.0f;  // -0.0 -> +0.0 (numpy sorts them as equal)
    if (s != s) return 0xFFFFFFFFu;   // NaN of either sign: np.argsort puts NaN last, the reference's [::-1] puts it FIRST (:454)
    uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// valid_scores = traditional_score * valid_regions (grasp_point_selector.py:451) -- a product, not a selection: a NaN or
// infinite score (non-finite depth on the leaf) stays NaN where the pixel is not valid, and NaN leads the candidate order
__device__ __forceinline__ float lg_valid_score(float trad, bool valid) { return trad * (valid ? 1.0f : 0.0f); }
// flatness of a tile off the leaf: exp(-flat_scale * |grad 0|), evaluated at run time (lg_final_kernel's constant path; top-k and
// the gather substitute it for tiles that path left unwritten, and must get the same float, whatever flat_scale is).  Its
// traditional score is w_flat * this, one multiplication.
__device__ __forceinline__ float lg_const_flat(float flat_scale) {
    float zero = 0.0f;
    asm volatile("" : "+v"(zero));
    return __expf(-flat_scale * __builtin_amdgcn_sqrtf(zero));
}
__device__ __forceinline__ int lg_reflect(int v, int n) {  // torch 'reflect' index, clamped for safety
    if (v < 0) v = -v;
    if (v >= n) v = 2 * (n - 1) - v;
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}
__device__ __forceinline__ float lg_uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// ---- the per-pixel arithmetic, stated once: lg_final_kernel and the deferred form of lg_gather_kernel both call these, so a
//      plane the gather computes at its windows is the float the plane kernel would have stored there.  hipcc contracts a * b + c
//      to an FMA where it likes, and the same inlined source did not contract alike in two kernels (sdf and the gradient's square
//      came out with the other product fused): contraction is therefore off in lg_flat4 and lg_pixels4 and every FMA is written
//      out -- in the form the plane kernel has been compiled to all along, so its planes keep their bits.
//      FROZEN HISTORY, NOT A NUMERICAL CHOICE: which product is fused where (pixel 0 of four unfused, f^2 fused for pixels 0-1,
//      FUSE_SY by instantiation) is what one compiler version happened to emit for the plane kernel before these functions
//      existed.  No form is more accurate than another; they are written down so that the planes, the patches and every test
//      that compares them byte for byte stay what they were.  Do not tidy them up.  The Gaussian taps below are NOT pinned
//      (see there): a toolchain change can still alter the last bit of flatness, in every kernel alike.
// Gaussian taps in ascending order, along a row (stride 1) and down a column (stride S floats)
// (These two stay under the compiler's contraction: inside lg_final_kernel's unrolled row loops it compiles them to a mixture of
// packed multiplies + adds and FMAs that depends on the row's place in the tile.  The smoothed plane, and with it flatness, can
// therefore not be recomputed bit for bit anywhere else without changing the plane kernel's own output: flatness stays a
// stored plane, profiles/NOTES_deferred_planes.md.)
template <int R>
__device__ __forceinline__ float lg_tap_row(const float (&kw)[2 * R + 1], const float* p) {
    float acc = kw[0] * p[0];
#pragma unroll
    for (int i = 1; i < 2 * R + 1; i++) acc += kw[i] * p[i];
    return acc;
}
template <int R, int S>
__device__ __forceinline__ float lg_tap_col(const float (&kw)[2 * R + 1], const float* p) {
    float acc = kw[0] * p[0];
#pragma unroll
    for (int i = 1; i < 2 * R + 1; i++) acc += kw[i] * p[i * S];
    return acc;
}
// flatness of four pixels x .. x + 3 of a row: Sobel cross-correlation on the smoothed, reflect-padded plane, exp(-scale |grad|)
// (:646-655).  ga, gb, gc: rows y - 1, y, y + 1 of that plane at columns x - 1 .. x + 4.  (2 * g is exact: the sums round the
// same fused or not.)  FUSE_SY: which square of sx^2 + sy^2 is fused -- the instantiations of the plane kernel had been compiled
// either way: every plane wanted and W % 4 == 0 fused sy, the others sx; the score-only form follows the dense call of its width.
template <bool FUSE_SY>
__device__ __forceinline__ void lg_flat4(const float (&ga)[6], const float (&gb)[6], const float (&gc)[6], float flat_scale,
                                         float (&o_flat)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float sx = (ga[j + 2] - ga[j]) + 2.0f * (gb[j + 2] - gb[j]) + (gc[j + 2] - gc[j]);
        float sy = (gc[j] + 2.0f * gc[j + 1] + gc[j + 2]) - (ga[j] + 2.0f * ga[j + 1] + ga[j + 2]);
        const float g2 = FUSE_SY ? __builtin_fmaf(sy, sy, sx * sx) : __builtin_fmaf(sx, sx, sy * sy);
        o_flat[j] = __expf(-flat_scale * __builtin_amdgcn_sqrtf(g2));  // v_sqrt_f32, 1 ulp
    }
}
// frame scalars of the per-pixel block.  AP: a pointer to the LgFinalArgs (the plane kernel's kernarg segment, or the
// gather's by-value copy); FP / MP: the frame's LgFrameParams and its two maxfix words
struct LgPixFrame {
    int has_angle;
    float sin_t, cos_t, inv_maxabs, opt_d, inv_2s2, focal, f2, ramp_step;
};
template <class AP, class FP, class MP>
__device__ __forceinline__ LgPixFrame lg_pix_frame(AP ap, FP fpp, MP mfp) {
    LgPixFrame c;
    c.has_angle = fpp->has_angle;
    c.sin_t = fpp->sin_t; c.cos_t = fpp->cos_t;
    const uint32_t mfi = mfp[0], mfo = mfp[1];
    const float maxabs = fmaxf((float)mfi * (1.0f / 65536.0f), (float)mfo * (1.0f / 65536.0f));
    c.inv_maxabs = lg_uniform_f(__frcp_rn(maxabs));
    c.opt_d = ap->optimal_distance;
    c.inv_2s2 = ap->inv_2s2;
    c.focal = ap->f;
    c.f2 = c.focal * c.focal;
    c.ramp_step = ap->iso_ramp_step;
    return c;
}
// the four pixels x0 .. x0 + 3 of row y on a wave that holds a leaf pixel: geometry, SDF / edge term, isolation (ISO: it is no
// part of `traditional`, the score-only plane kernel leaves it out), fusion, validity.  mnib / snib: their mask and stem bits;
// din: distance_map; o_flat: lg_flat4.  Returns the validity bytes (bit 8 j: pixel j).
// Which products are fused is the plane kernel's compiled form, by the pixel's place x & 3 in its lane's four (x0 % 4 == 0
// there; the gather's groups start anywhere): pixel 0 rounds dx^2 and dy^2 separately (they were one packed multiply), pixels
// 1-3 fuse dx^2; pixels 0-1 fuse f^2 into r^2 + f^2, pixels 2-3 add the rounded f^2.
template <bool ISO, class AP>
__device__ __forceinline__ uint32_t lg_pixels4(AP ap, const LgPixFrame& c, int y, int x0, int H, int W, unsigned mnib, unsigned snib,
                                               const float* din, const float (&o_flat)[4], float w_flat, float (&o_sdf)[4],
                                               float (&o_app)[4], float (&o_iso)[4], float (&o_acc)[4], float (&o_stem)[4],
                                               float (&o_trad)[4], bool (&o_valid)[4]) {
#pragma clang fp contract(off)
    uint32_t vbytes = 0;
    const float dyp = (float)(y - ap->cyi) - ap->cyf;  // exact integer part first: no cancellation near the centre
    const float dyp2 = dyp * dyp;
    const int dyb = min(y + 1, H - y);
    const float ramp = __builtin_fmaf(c.ramp_step, (float)y, ap->iso_ramp_top);
    const float w_approach = ap->w_approach, w_sdf = ap->w_sdf, w_access = ap->w_access;
    const int has_angle = c.has_angle;
    const float sin_t = c.sin_t, cos_t = c.cos_t, inv_maxabs = c.inv_maxabs, opt_d = c.opt_d, inv_2s2 = c.inv_2s2;
    const float focal = c.focal, f2 = c.f2;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = x0 + j;
        const float m = ((mnib >> j) & 1u) ? 1.0f : 0.0f;
        const float st = ((snib >> j) & 1u) ? 1.0f : 0.0f;
        // closed-form geometry planes                                           (:502-524, :569-593)
        const float dxp = (float)(x - ap->cxi) - ap->cxf;
        const int jj = x & 3;
        const float r2 = jj == 0 ? dxp * dxp + dyp2 : __builtin_fmaf(dxp, dxp, dyp2);
        const float inv_r = r2 > 0.0f ? rsqrtf(r2) : 0.0f;
        const float r = r2 * inv_r;
        const float r2f2 = jj < 2 ? __builtin_fmaf(focal, focal, r2) : f2 + r2;
        const float app = focal * rsqrtf(r2f2) * m;
        const float cosang = r2 > 0.0f ? dxp * inv_r : 1.0f;
        const float acc = __builtin_fmaf(ap->access_w_dir, cosang, ap->access_w_dist * __builtin_fmaf(-ap->inv_maxd, r, 1.0f)) * m;
        // SDF / edge term                                                        (:526-567)
        const float align = has_angle ? fabsf(__builtin_fmaf(sin_t, dxp * inv_r, -(cos_t * (dyp * inv_r)))) : 1.0f;
        const float dd = din[j] - opt_d;
        const float interior = __expf(-(dd * dd) * inv_2s2);
        const float sdfn = din[j] * inv_maxabs;  // inside the mask d_out == 0
        const float sdf = __builtin_fmaf(ap->sdf_w_sdf, sdfn, __builtin_fmaf(ap->sdf_w_interior, interior, ap->sdf_w_align * align)) * m;
        float iso = 0.0f;
        if (ISO) {
            // degenerate isolation map: chamfer-3 transform of an image with no zero pixel (:595-633)
            const int dbrd = min(min(x + 1, W - x), dyb);
            const float dt3 = (float)(ap->init0 + (uint32_t)dbrd * LG_A3) * (1.0f / 65536.0f);
            const float s = dt3 * ap->iso_inv_max;
            iso = __builtin_fmaf(ap->iso_w_close, s, ap->iso_w_wide * s) * ramp * m;
        }
        // fusion + validity                                                      (:272-288)
        const float trad = __builtin_fmaf(w_access, acc, __builtin_fmaf(w_flat, o_flat[j], __builtin_fmaf(w_approach, app, w_sdf * sdf))) *
                           (1.0f - st);
        const bool valid = (din[j] > ap->min_edge_distance) && (m > 0.0f) && (st < ap->stem_valid_thresh);
        o_sdf[j] = sdf; o_app[j] = app; o_iso[j] = iso; o_acc[j] = acc; o_stem[j] = st; o_trad[j] = trad;
        o_valid[j] = valid;
        if (valid) vbytes |= 1u << (8 * j);
    }
    return vbytes;
}
