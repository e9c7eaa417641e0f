"""CollectingGraspPointSelector -- mirror of the select_grasp_point that feeds the data collector
(scripts/utils/grasp_point_selector_bkp.py:73-169, the only caller of collect_sample in the reference).

It differs from GraspPointSelector.select_grasp_point: the leaf is eroded twice by a 21 x 21 ellipse into a safe zone, the
planes are computed on that zone (flatness alone on depth * the original mask), a tip-penalty term stands where the
accessibility term stood, the point is the plain arg-max of the fused plane with the centroid of the original mask behind it,
and the score planes, the point and np.max(traditional_score) go to `data_collector.collect_sample`.  All per-pixel work is one
library call (lg_select_grasp_collect, include/leafgrasp.h); tensors stay on the device.
"""
import ctypes as C

import torch

from ._lib import MAP_NAMES, LgCollectParams, LgGraspResult, LgParams, check, lib
from ._log import logerr, loginfo
from .grasp_point_selector import GraspPointSelector, _triples

_VP = C.c_void_p


def default_collect_params():
    p = LgCollectParams()
    lib.lg_default_collect_params(C.byref(p))
    return p


class CollectingGraspPointSelector(GraspPointSelector):
    """The variant's constructor fields (bkp:17-34): erosion_kernel_size, erosion_iterations, min_edge_distance, the camera
    fields, data_collector (None: select without collecting) and ml_predictor = None -- the variant's ML branch needs a
    predictor class the reference no longer has and is not part of this class.
    tip_aware (keyword, also per call): False = the tip penalty as written; True = the method's stated intent, which the
    library does not build yet (the call fails with LG_ERR_UNSUPPORTED, i.e. the logged None triple)."""

    def __init__(self, device, data_collector=None, tip_aware=False):
        super().__init__(device, load_model=False)
        self.data_collector = data_collector
        self.tip_aware = bool(tip_aware)
        self.collect_params = default_collect_params()
        self.erosion_kernel_size = self.collect_params.erosion_kernel_size   # 21 (bkp:30)
        self.erosion_iterations = self.collect_params.erosion_iterations     # 2  (bkp:31)

    def _sync_collect_params(self, tip_aware=None):
        cp = LgCollectParams.from_buffer_copy(self.collect_params)
        cp.erosion_kernel_size = int(self.erosion_kernel_size)
        cp.erosion_iterations = int(self.erosion_iterations)
        cp.tip_aware = 1 if (self.tip_aware if tip_aware is None else tip_aware) else 0
        return cp

    def _prep_mask(self, masks):
        m = (masks if torch.is_tensor(masks) else torch.as_tensor(masks)).to(self.device)
        if m.dtype == torch.bool:
            m = m.contiguous().view(torch.uint8)
        elif m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
        m = m.contiguous()
        if m.dim() == 2:
            m = m.unsqueeze(0)
        if m.dim() != 3:
            raise ValueError(f"mask {tuple(m.shape)} must be [H,W] or [B,H,W]")
        return m

    # ------------------------------------------------------------------ the stages on their own
    def erode(self, leaf_masks, kernel_size=None, iterations=None):
        """cv2.erode(mask, ellipse(kernel_size), iterations=iterations) on the device (lg_erode_ellipse): [H,W] or [B,H,W] u8 /
        bool in, a uint8 0 / 1 tensor of the same shape out.  Defaults: the selector's erosion fields."""
        m = self._prep_mask(leaf_masks)
        B, H, W = m.shape
        out = torch.empty_like(m)
        k = self.erosion_kernel_size if kernel_size is None else kernel_size
        it = self.erosion_iterations if iterations is None else iterations
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_erode_ellipse(self._h, m.data_ptr(), B, H, W, int(k), int(it), out.data_ptr(), self._stream()),
                  "lg_erode_ellipse")
        return out[0] if getattr(leaf_masks, "ndim", 3) == 2 else out

    def tip_penalty(self, safe_masks, tip_aware=None):
        """The tip-penalty plane of given safe zones (lg_tip_penalty): float32, same shape."""
        m = self._prep_mask(safe_masks)
        B, H, W = m.shape
        out = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        p, cp = LgParams.from_buffer_copy(self.params), self._sync_collect_params(tip_aware)
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_tip_penalty(self._h, m.data_ptr(), B, H, W, C.byref(p), C.byref(cp), out.data_ptr(), None,
                                              self._stream()), "lg_tip_penalty")
        return out[0] if getattr(safe_masks, "ndim", 3) == 2 else out

    def argmax_first(self, planes):
        """np.argmax per frame of float32 planes on the device (lg_argmax_first): lists of (x, y), np.max and (plane > 0).any()."""
        t = torch.as_tensor(planes).to(self.device, torch.float32).contiguous()
        t3 = t.unsqueeze(0) if t.dim() == 2 else t
        B, H, W = t3.shape
        xy, mx, anyp = (C.c_int32 * (2 * B))(), (C.c_float * B)(), (C.c_int32 * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_argmax_first(self._h, t3.data_ptr(), B, H, W, xy, mx, anyp, self._stream()), "lg_argmax_first")
        return [(xy[2 * b], xy[2 * b + 1]) for b in range(B)], [float(v) for v in mx], [bool(v) for v in anyp]

    # ------------------------------------------------------------------ the path (bkp:73-169)
    def select_grasp_points_batch(self, leaf_masks, depth_tensors, return_maps=False, image_processor=None, tip_aware=None):
        """B frames at once, without collection.  Returns the list of (xy, XYZ, preXYZ) triples; with return_maps also the dict of
        device planes (the eight names of MAP_NAMES computed as the variant computes them, plus 'tip_penalty'), the validity
        plane and the safe zone (uint8 [B,H,W] each).  Bad input raises."""
        m, d, _ = self._prep_inputs(leaf_masks, depth_tensors)
        B, H, W = m.shape
        p = LgParams.from_buffer_copy(self._sync_params(image_processor))
        cp = self._sync_collect_params(tip_aware)
        maps = tip = valid = safe = None
        ptrs = None
        if return_maps:
            maps, ptrs = self._alloc_maps(B, H, W)
            tip = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
            valid = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
            safe = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        res = (LgGraspResult * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_select_grasp_collect(
                self._h, d.data_ptr(), m.data_ptr(), B, H, W, C.byref(p), C.byref(cp), C.byref(ptrs) if ptrs is not None else None,
                tip.data_ptr() if return_maps else None, safe.data_ptr() if return_maps else None,
                valid.data_ptr() if return_maps else None, res, self._stream()), "lg_select_grasp_collect")
        self.last_results = res
        out = _triples(res, B)
        if return_maps:
            planes = {n: maps[i] for i, n in enumerate(MAP_NAMES)}
            planes["tip_penalty"] = tip
            return out, planes, valid, safe
        return out

    def select_grasp_point(self, leaf_mask, depth_tensor, image_processor=None, pcl_data=None, tip_aware=None):
        """The reference's triple.  With a collector attached the frame's planes, the point and np.max(traditional_score) go to
        collect_sample(leaf_mask, depth_tensor, None, scores, point, best_score).  Never raises: errors are logged and give
        (None, None, None) -- an empty mask among them (the reference's centroid is NaN there and int() raises, twice)."""
        try:
            if self.data_collector is None:
                res = self.select_grasp_points_batch(leaf_mask, depth_tensor, image_processor=image_processor, tip_aware=tip_aware)[0]
                planes = None
            else:
                out, planes, _, _ = self.select_grasp_points_batch(leaf_mask, depth_tensor, return_maps=True,
                                                                   image_processor=image_processor, tip_aware=tip_aware)
                res = out[0]
            if res[0] is None:
                raise ValueError("cannot convert float NaN to integer (empty leaf mask: no centroid)")
            if pcl_data is not None:   # get_3d_grasp_point reads self.width, which the class never defines (bkp:58): quirk 10
                raise AttributeError("'GraspPointSelector' object has no attribute 'width'")
            if planes is not None:
                scores = {n: t[0] for n, t in planes.items() if n != "traditional_score"}
                best = float(self.last_results[0].best_score)
                if self.data_collector.collect_sample(leaf_mask, depth_tensor, None, scores, res[0], best):
                    loginfo("Collected training sample")
            return res
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in grasp point selection: {str(e)}")
            return None, None, None
