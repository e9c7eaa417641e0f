"""GraspPointSelector -- drop-in mirror of scripts/utils/grasp_point_selector.py::GraspPointSelector.

Same constructor, attributes (`camera_cx`, `camera_cy`, `f_norm`), method names, argument order, return
shapes and error convention (never raise across `select_grasp_point`: log and return (None, None, None),
grasp_point_selector.py:251-253).  All per-pixel work runs in liblgrasp.so (hand-written gfx950 HIP) through
the C-ABI in include/leafgrasp.h; tensors stay on the GPU and are handed over as raw device pointers.
There is no CPU fallback: constructing a selector without a HIP device raises.
"""
import ctypes as C
import math
import os
import threading

import numpy as np
import torch

from . import _lib
from ._lib import LG_NUM_MAPS, MAP_NAMES, LgGraspCandidate, LgGraspResult, LgMlSample, LgMlSampling, LgParams, check, lib
from ._log import logerr, loginfo, logwarn
from .cnn import pack_state_dict
from .image_processor import flatness_config

# LgGraspResult rows as a numpy record (select_grasp_points_batch reads whole columns)
_RESULT_DTYPE = np.dtype([(n, np.int32 if t is C.c_int else np.float32) for n, t in LgGraspResult._fields_])
assert _RESULT_DTYPE.itemsize == C.sizeof(LgGraspResult)
# lg_grasp_candidate rows (select_grasp_candidates_batch returns them as a [B, top_k] array of this dtype)
GRASP_CANDIDATE_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.float32) for n, t in LgGraspCandidate._fields_])
assert GRASP_CANDIDATE_DTYPE.itemsize == C.sizeof(LgGraspCandidate)
_ML_FIELDS = ("ml_score", "ml_confidence", "combined")
# lg_ml_sample rows (select_grasp_points_ml_batch(return_samples=True) returns a [B, max_samples] array of this dtype)
ML_SAMPLE_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.float32) for n, t in LgMlSample._fields_])
assert ML_SAMPLE_DTYPE.itemsize == C.sizeof(LgMlSample) == 20

_VP = C.c_void_p

# status words of lg_detect_midrib
MIDRIB_FOUND, MIDRIB_NO_CONTOUR, MIDRIB_THIN, MIDRIB_TOO_FEW = 0, 1, 2, 3


def _device_index(device):
    d = torch.device(device) if not isinstance(device, torch.device) else device
    if d.type != "cuda":
        raise RuntimeError(
            f"leafgrasp_amd needs a HIP device (got device '{d}'): the grasp-scoring path has no CPU fallback")
    return d.index if d.index is not None else torch.cuda.current_device()


class GraspPointSelector:
    def __init__(self, device, load_model=True):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        # scoring weights / parameters kept as attributes like the reference (grasp_point_selector.py:17-33)
        self.flatness_weight = 0.25
        self.isolation_weight = 0.4
        self.edge_weight = 0.2
        self.accessibility_weight = 0.15
        self.min_flat_area_size = 15
        self.min_edge_distance = 20
        self.isolation_radius = 50
        self.camera_cx = 707
        self.camera_cy = 494
        self.f_norm = None
        self.erosion_kernel_size = 21
        self.erosion_iterations = 2
        self.params = _lib.default_params()
        self._h = _VP()
        self._dev_index = _device_index(self.device)
        check(None, lib.lg_create(self._dev_index, C.byref(self._h)), "lg_create")
        self.ml_predictor = None  # truthy object when CNN weights are loaded (reference attribute name)
        self._keep = None
        if load_model:
            self.load_ml_model()

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                lib.lg_destroy(self._h)
                self._h = _VP()
        except Exception:  # noqa: BLE001
            pass

    # ------------------------------------------------------------------ model (grasp_point_selector.py:43-57)
    def load_ml_model(self, model_path=None):
        """Load trained CNN weights from ~/leaf_grasp_output/ml_models/best_model.pth (key
        'model_state_dict'); absent file => traditional scoring only, exactly like the reference."""
        try:
            model_path = model_path or os.path.expanduser("~/leaf_grasp_output/ml_models/best_model.pth")
            if os.path.exists(model_path):
                checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
                self.set_cnn_state_dict(checkpoint["model_state_dict"])
                loginfo("Loaded ML grasp model")
            else:
                logwarn("No ML model found, will use traditional scoring only")
                self.ml_predictor = None
        except Exception as e:  # noqa: BLE001
            logerr(f"Error loading ML model: {str(e)}")
            self.ml_predictor = None

    def set_cnn_state_dict(self, state_dict):
        """Install GraspPointCNN weights (state_dict of the reference module; BN is folded in the library)."""
        w, keep = pack_state_dict(state_dict)
        check(self._h, lib.lg_cnn_load(self._h, C.byref(w)), "lg_cnn_load")
        self._keep = keep
        self.ml_predictor = "lg_cnn"

    def load_from_trainer(self, trainer):
        """Install the weights a GraspTrainer holds right now, on the device (lg_cnn_load_from_trainer): the same floats as
        set_cnn_state_dict(trainer.state_dict()), without the state dict.  The call orders itself after the trainer's steps;
        a model of the same geometry is refreshed in place.  A model the inference kernels do not take (LgError, status
        LG_ERR_UNSUPPORTED) leaves the loaded one as it is."""
        th = getattr(trainer, "_h", None)
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_cnn_load_from_trainer(self._h, th if th else None), "lg_cnn_load_from_trainer")
        self._keep = None
        self.ml_predictor = "lg_cnn"

    def cnn_weights(self, which, layer=0):
        """Inspection: one weight buffer of the loaded CNN as the kernels read it (lg_debug_cnn_weights; `which`: a key of
        _lib.CNNW), float32 numpy array, empty when the model has no such buffer.  'allocs': the number of weight buffers
        set_cnn_state_dict and load_from_trainer have allocated on this selector so far (an int; an in-place refresh by
        load_from_trainer adds none)."""
        n = C.c_int64()
        code = _lib.CNNW[which]
        check(self._h, lib.lg_debug_cnn_weights(self._h, code, int(layer), None, 0, C.byref(n)), "lg_debug_cnn_weights")
        if which == "allocs":
            return int(n.value)
        out = np.empty(n.value, np.float32)
        if n.value:
            check(self._h, lib.lg_debug_cnn_weights(self._h, code, int(layer), out.ctypes.data_as(C.POINTER(C.c_float)), out.size,
                                                    C.byref(n)), "lg_debug_cnn_weights")
        return out

    def eval_logits(self, logits, labels, batch_size=16, pos_weight=2.0, threshold=0.5):
        """Validation loss and counts of device logits (lg_eval_logits) -> _lib.LgEvalResult."""
        z = torch.as_tensor(logits).to(self.device, torch.float32).contiguous().reshape(-1)
        y = torch.as_tensor(labels).to(self.device, torch.float32).contiguous().reshape(-1)
        if z.shape != y.shape:
            raise ValueError("logits and labels must have the same length")
        r = _lib.LgEvalResult()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_eval_logits(self._h, z.data_ptr(), y.data_ptr(), int(z.shape[0]), int(batch_size),
                                              float(pos_weight), float(threshold), C.byref(r), self._stream()), "lg_eval_logits")
        return r

    def evaluate(self, features, labels, batch_size=16, pos_weight=2.0, threshold=0.5, return_logits=False):
        """The validation pass of train_model.py:280-311 on the loaded CNN in one call (lg_cnn_evaluate): forward, per-batch
        BCEWithLogitsLoss(pos_weight) averaged over the batches, accuracy and analyze_predictions' metrics (threshold on the
        logit).  features [N,9,32,32], labels [N].  Returns {"val_loss", "accuracy" (percent), "n", "metrics"[, "logits"]}."""
        from .trainer import metrics_from_counts
        x = torch.as_tensor(features).to(self.device, torch.float32).contiguous()
        y = torch.as_tensor(labels).to(self.device, torch.float32).contiguous().reshape(-1)
        N = int(x.shape[0])
        if tuple(x.shape) != (N, 9, 32, 32) or tuple(y.shape) != (N,):
            raise ValueError("features must be [N,9,32,32] and labels [N]")
        logits = torch.empty((N,), dtype=torch.float32, device=self.device) if return_logits else None
        r = _lib.LgEvalResult()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_cnn_evaluate(self._h, x.data_ptr(), y.data_ptr(), N, int(batch_size), float(pos_weight),
                                               float(threshold), logits.data_ptr() if return_logits else None, C.byref(r),
                                               self._stream()), "lg_cnn_evaluate")
        out = {"val_loss": float(r.loss), "accuracy": 100.0 * r.correct / r.n, "n": int(r.n),
               "metrics": metrics_from_counts(int(r.tp), int(r.fp), int(r.fn), int(r.tn))}
        if return_logits:
            out["logits"] = logits
        return out

    def clear_cnn(self):
        lib.lg_cnn_unload(self._h)
        self.ml_predictor = None

    # ------------------------------------------------------------------ camera (:145-150)
    def set_camera_params(self, projection_matrix):
        self.f_norm = projection_matrix[0, 0]
        self.camera_cx = projection_matrix[0, 2]
        self.camera_cy = projection_matrix[1, 2]
        self.baseline = -projection_matrix[0, 3] / self.f_norm

    def _sync_params(self, image_processor=None):
        if self.f_norm is None:
            # reference: np.full(..., None) in calculate_approach_vector_score raises -> caught -> None triple
            raise RuntimeError("camera parameters not set (f_norm is None): call set_camera_params first")
        p = self.params
        p.cx, p.cy, p.f = float(self.camera_cx), float(self.camera_cy), float(self.f_norm)
        p.min_edge_distance = float(self.min_edge_distance)
        # _calculate_flatness_map smooths with the CALLER's ImageProcessor (:635-657 -> image_processor.py:56-64): its
        # Gaussian size goes into lg_params (1 / 3 / 5 / 7; anything else is refused by the library, an even size fails in
        # the reference as well).  None (not possible in the reference) = the node's size 5.
        p.gaussian_size = 5 if image_processor is None else flatness_config(image_processor)
        return p

    # ------------------------------------------------------------------ tensors
    def _prep_inputs(self, leaf_mask, depth_tensor):
        if isinstance(leaf_mask, np.ndarray):
            leaf_mask = torch.from_numpy(leaf_mask)
        if isinstance(depth_tensor, np.ndarray):
            depth_tensor = torch.from_numpy(depth_tensor)
        is_bool = leaf_mask.dtype == torch.bool
        m = leaf_mask.to(self.device)
        if is_bool:
            m = m.contiguous().view(torch.uint8)  # bool storage is one 0/1 byte: reinterpret, no kernel
        elif m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
        m = m.contiguous()
        d = depth_tensor.to(self.device, torch.float32).contiguous()
        if m.dim() == 2:
            m, d = m.unsqueeze(0), d.unsqueeze(0)
        if m.shape != d.shape or m.dim() != 3:
            raise ValueError(f"mask {tuple(m.shape)} and depth {tuple(d.shape)} must both be [H,W] or [B,H,W]")
        return m, d, is_bool

    def _stream(self):
        return _VP(torch.cuda.current_stream(self.device).cuda_stream)

    def _alloc_maps(self, B, H, W, names=MAP_NAMES):
        maps = torch.empty((LG_NUM_MAPS, B, H, W), dtype=torch.float32, device=self.device)
        ptrs = (_VP * LG_NUM_MAPS)()
        for i, n in enumerate(MAP_NAMES):
            ptrs[i] = maps[i].data_ptr() if n in names else None
        return maps, ptrs

    # ------------------------------------------------------------------ score planes (:256-288)
    def score_maps(self, leaf_mask, depth_tensor, image_processor=None):
        """All eight planes + validity mask, device resident.
        Returns (dict name -> float32 tensor [B,H,W] or [H,W], valid uint8 tensor, theta list)."""
        m, d, _ = self._prep_inputs(leaf_mask, depth_tensor)
        B, H, W = m.shape
        p = self._sync_params(image_processor)
        maps, ptrs = self._alloc_maps(B, H, W)
        valid = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        theta = (C.c_float * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_score_maps(self._h, d.data_ptr(), m.data_ptr(), B, H, W, C.byref(p), C.byref(ptrs),
                                             valid.data_ptr(), theta, self._stream()), "lg_score_maps")
        squeeze = (leaf_mask.dim() if hasattr(leaf_mask, "dim") else leaf_mask.ndim) == 2
        out = {n: (maps[i, 0] if squeeze else maps[i]) for i, n in enumerate(MAP_NAMES)}
        th = [None if math.isnan(t) else float(t) for t in theta]
        return out, (valid[0] if squeeze else valid), (th[0] if squeeze else th)

    def dt_maxima(self, frame=0):
        """Inspection: (max d_in, max d_out) of `frame` in the last call, as float32 like cv2's planes
        (grasp_point_selector.py:529-533), and the sweep window (x0, x1, y0, y1) the distance transforms ran on."""
        import ctypes as C
        out, win = (C.c_uint32 * 2)(), (C.c_int32 * 4)()
        rc = lib.lg_debug_dt_max(self._h, int(frame), out, win)
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        scale = np.float32(1.0 / 65536.0)
        return np.float32(out[0]) * scale, np.float32(out[1]) * scale, tuple(win)

    def dt_form(self, frame=0):
        """Inspection: (searched, d_out sweeps skipped) of `frame` in the last call -- whether its d_in came from the row search
        or from the two sweeps is decided per batch on the device."""
        import ctypes as C
        form = (C.c_int32 * 2)()
        rc = lib.lg_debug_dt_form(self._h, int(frame), form)
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return bool(form[0]), bool(form[1])

    def dt_search_form(self):
        """Inspection: the form of the row search the last call queued for its searched frames (dt_form(i)[0]), in
        LG_DT_SEARCH_ALGO's numbering: 1 = one level, 5 = seed row pairs + stencil bands, 6 = one register sweep per frame; 0: no
        search is queued."""
        import ctypes as C
        algo = C.c_int32()
        rc = lib.lg_debug_dt_search_form(self._h, C.byref(algo))
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return int(algo.value)

    def options(self):
        """Inspection: the experiment switches as this handle found them when it was created (lg_debug_options), name -> int."""
        buf = C.create_string_buffer(4096)
        n = lib.lg_debug_options(self._h, buf, len(buf))
        if not 0 < n < len(buf):
            raise RuntimeError(f"lg_debug_options -> {n}")
        return {k: int(v) for k, v in (ln.split("=") for ln in buf.value.decode().splitlines())}

    def cnn_scored(self):
        """Inspection: how many patches the last select_grasp_point(s) / select_grasp_candidates call put through the CNN --
        the candidates that could still beat candidate 0 (lg_cnn_candidate_cannot_win), or every one (B * top_k) for the
        candidates entry and with LG_CNN_PRUNE=0."""
        n = C.c_int64()
        rc = lib.lg_debug_cnn_scored(self._h, C.byref(n))
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return int(n.value)

    def cnn_survivors(self):
        """Inspection: the CNN pass of the last select_grasp_point(s) / select_grasp_candidates call, patch by patch
        (lg_debug_cnn_survivors).  Returns a dict: sub_frames, n_sub (the call's sub-batches; one of B frames by default),
        counts [n_sub] (patches each sub-batch put through the CNN), and list, slot (int32) and logits (float32), each
        [B * top_k] with sub-batch k's entries from k * sub_frames * top_k on and indices counted from there: list[j] = frame *
        top_k + candidate of patch j (-1 past the count), slot[frame * top_k + candidate] = its patch or -1 (pruned), logits[j]
        = the logit of patch j (stale past the count).  The identity where every candidate is scored."""
        sub_frames, n_sub, n_slots = C.c_int32(), C.c_int32(), C.c_int64()
        i32 = C.POINTER(C.c_int32)
        rc = lib.lg_debug_cnn_survivors(self._h, C.byref(sub_frames), C.byref(n_sub), None, 0, None, None, None, 0,
                                        C.byref(n_slots))   # the sizes
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        n = int(n_slots.value)
        counts = np.zeros(int(n_sub.value), np.int32)
        lst, slot, logits = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        rc = lib.lg_debug_cnn_survivors(self._h, C.byref(sub_frames), C.byref(n_sub), counts.ctypes.data_as(i32), counts.size,
                                        lst.ctypes.data_as(i32), slot.ctypes.data_as(i32),
                                        logits.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(n_slots))
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return dict(sub_frames=int(sub_frames.value), n_sub=int(n_sub.value), counts=counts, list=lst, slot=slot, logits=logits)

    def tail_lanes(self, lanes=None):
        """Inspection and control of the tail lanes (lg_debug_tail_lanes): lanes = 0 the automatic rule, 1 .. 4 that many lanes
        wherever a call may run in lanes, None only reports.  Returns the lanes of the last select_grasp_point(s) call on this
        selector (1: it did not run in lanes; 0: none yet).  Results never depend on the lanes."""
        last = C.c_int32()
        rc = lib.lg_debug_tail_lanes(self._h, -1 if lanes is None else int(lanes), C.byref(last))
        if rc != 0:
            raise RuntimeError(f"lg_debug_tail_lanes({lanes}) -> {rc}")
        return int(last.value)

    def patch(self, slot):
        """Inspection: [9, 32, 32] float32, the patch in slot `slot` of the last select call with a model loaded, as the CNN read
        it (lg_debug_patch; slots as in cnn_survivors()['list'])."""
        out = np.zeros((9, 32, 32), np.float32)
        rc = lib.lg_debug_patch(self._h, int(slot), out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return out

    def isolation_fields(self, frame, H, W):
        """Inspection: (dc_fix, dw_fix, (max_c, max_w)) of frame `frame` of the last label-aware select call -- the raw 16.16
        chamfer-3 transforms over the whole [H, W] frame and their maxima (lg_debug_isolation_fields) -- or None for a frame
        without another leaf (it took the closed form)."""
        dc, dw = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
        mx = (C.c_uint32 * 2)()
        rc = lib.lg_debug_isolation_fields(self._h, int(frame), dc.ctypes.data, dw.ctypes.data, mx)
        if rc < 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return (dc, dw, (int(mx[0]), int(mx[1]))) if rc == 1 else None

    def ws_plane_bytes(self):
        """Inspection: dict plane name -> bytes of device memory this handle holds for its own copy of that plane
        (lg_debug_ws_plane_bytes).  A selector that has only made calls without return_maps holds distance_map,
        traditional_score and flatness_map only."""
        b = (C.c_int64 * LG_NUM_MAPS)()
        rc = lib.lg_debug_ws_plane_bytes(self._h, b)
        if rc != 0:
            raise RuntimeError(lib.lg_last_error(self._h).decode())
        return {n: int(b[i]) for i, n in enumerate(MAP_NAMES)}

    def _calculate_all_scores(self, leaf_mask_np, depth_tensor, image_processor=None):
        """Reference signature (:256): numpy uint8 mask in, dict of numpy planes out."""
        out, _, _ = self.score_maps(leaf_mask_np, depth_tensor, image_processor)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def _get_valid_regions(self, leaf_mask_np, scores):  # :282-288 (host helper for callers holding a scores dict)
        return ((scores["distance_map"] > self.min_edge_distance) & (np.asarray(leaf_mask_np) > 0)
                & (scores["stem_penalty"] < self.params.stem_valid_thresh))

    # ------------------------------------------------------------------ candidates (:447-482)
    def _get_candidate_points(self, score_map, valid_regions, top_k=20, min_distance=10):
        try:
            sm = torch.as_tensor(np.asarray(score_map, dtype=np.float32) if not torch.is_tensor(score_map) else score_map)
            vr = torch.as_tensor(np.asarray(valid_regions) if not torch.is_tensor(valid_regions) else valid_regions)
            sm = sm.to(self.device, torch.float32).contiguous()
            vr = (vr.to(self.device) != 0).to(torch.uint8).contiguous()
            if sm.dim() == 2:
                sm, vr = sm.unsqueeze(0), vr.unsqueeze(0)
            B, H, W = sm.shape
            xy = torch.zeros((B, top_k, 2), dtype=torch.int32, device=self.device)
            n = torch.zeros((B,), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                check(self._h, lib.lg_topk_nms(self._h, sm.data_ptr(), vr.data_ptr(), B, H, W, int(top_k),
                                               int(min_distance), xy.data_ptr(), n.data_ptr(), self._stream()),
                      "lg_topk_nms")
            xy, n = xy.cpu().numpy(), n.cpu().numpy()
            res = [[(int(xy[b, i, 0]), int(xy[b, i, 1])) for i in range(int(n[b]))] for b in range(B)]
            return res[0] if B == 1 else res
        except Exception as e:  # noqa: BLE001
            logerr(f"Error getting candidate points: {str(e)}")
            return []

    # ------------------------------------------------------------------ patches + CNN (:59-143)
    def gather_patches(self, leaf_mask, depth_tensor, maps, points):
        """[len(points), 9, 32, 32] float32 device tensor of normalised patches (single frame)."""
        m, d, _ = self._prep_inputs(leaf_mask, depth_tensor)
        _, H, W = m.shape
        k = len(points)
        xy = torch.tensor(points, dtype=torch.int32, device=self.device).reshape(1, k, 2).contiguous()
        n = torch.tensor([k], dtype=torch.int32, device=self.device)
        ptrs = (_VP * LG_NUM_MAPS)()
        keep = []
        for i, name in enumerate(MAP_NAMES):
            t = maps[name]
            t = torch.as_tensor(t).to(self.device, torch.float32).contiguous()
            keep.append(t)
            ptrs[i] = t.data_ptr()
        patches = torch.empty((1, k, 9, 32, 32), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_gather_patches(self._h, d.data_ptr(), m.data_ptr(), C.byref(ptrs), 1, H, W, k,
                                                 xy.data_ptr(), n.data_ptr(), patches.data_ptr(), self._stream()),
                  "lg_gather_patches")
            torch.cuda.current_stream(self.device).synchronize()
        return patches[0]

    def cnn_forward(self, patches):
        """GraspPointCNN logits for [N,9,32,32] float32 patches (device tensor)."""
        x = torch.as_tensor(patches).to(self.device, torch.float32).contiguous()
        N = x.shape[0]
        logits = torch.empty((N,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_cnn_forward(self._h, x.data_ptr(), N, logits.data_ptr(), self._stream()),
                  "lg_cnn_forward")
        return logits

    def get_ml_score(self, leaf_mask, depth_tensor, scores, point):
        """Reference signature (:59): CNN score of one point, None when no model / on error."""
        try:
            if self.ml_predictor is None:
                return None
            x, y = point
            m = torch.as_tensor(leaf_mask)
            H, W = m.shape[-2:]
            if m.dtype == torch.bool and (x < 16 or y < 16 or x + 16 > W or y + 16 > H):
                logwarn(f"Failed to extract mask patch at ({x}, {y})")
                return None
            patches = self.gather_patches(leaf_mask, depth_tensor, scores, [(int(x), int(y))])
            logit = float(self.cnn_forward(patches)[0])
            s = 1.0 / (1.0 + math.exp(-logit))
            return float(np.tanh(s * 3.0) * 0.5 + 0.5)
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in ML scoring: {str(e)}")
            return None

    # ------------------------------------------------------------------ the path (:184-253)
    def select_grasp_points_batch(self, leaf_masks, depth_tensors, return_maps=False, image_processor=None):
        """B frames at once ([B,H,W] mask + depth).  Returns a list of (xy, XYZ, preXYZ) triples."""
        m, d, is_bool = self._prep_inputs(leaf_masks, depth_tensors)
        B, H, W = m.shape
        p = self._sync_params(image_processor)
        p.mask_is_bool = 1 if is_bool else 0
        maps = valid = None
        ptrs = None
        vptr = None
        if return_maps:
            maps, ptrs = self._alloc_maps(B, H, W)
            valid = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
            vptr = valid.data_ptr()
        res = (LgGraspResult * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_select_grasp(self._h, d.data_ptr(), m.data_ptr(), B, H, W, C.byref(p),
                                               C.byref(ptrs) if ptrs is not None else None, vptr, res,
                                               self._stream()), "lg_select_grasp")
        out = _triples(res, B)
        self.last_results = res
        if return_maps:
            return out, {n: maps[i] for i, n in enumerate(MAP_NAMES)}, valid
        return out

    def select_grasp_points_for_leaves(self, label_tensors, leaf_ids, depth_tensors, image_processor=None, label_aware=False):
        """select_grasp_points_batch(label_tensors == leaf_ids[:, None, None], depth_tensors) -- the node's `optimal_mask =
        mask_tensor == optimal_leaf_id` and select_grasp_point (leaf_grasp_node_v3.py:118-125) -- with the comparison folded into
        the library's first pass over the frames (lg_select_grasp_labels).  label_tensors: [B,H,W] int16 on this device; leaf_ids:
        B ints, None for a frame without a leaf (the node does not call select_grasp_point for it: its triple is (None, None,
        None)).  The mask counts as the torch.bool tensor the node passes.
        label_aware=True (lg_params.label_aware): the isolation map and the pre-grasp clearance see the other leaves of the
        label image (every label > 0 that is not the frame's leaf) instead of the one leaf alone; a frame without another leaf
        keeps its results.  The CNN then sees another channel 5: retrain a model that was trained on the degenerate one."""
        lab = label_tensors
        if not (torch.is_tensor(lab) and lab.dtype == torch.int16 and lab.is_cuda and lab.dim() == 3 and lab.is_contiguous()):
            raise ValueError("label_tensors must be a contiguous [B,H,W] int16 tensor on the device")
        d = depth_tensors.to(self.device, torch.float32).contiguous()
        if d.shape != lab.shape:
            raise ValueError(f"labels {tuple(lab.shape)} and depth {tuple(d.shape)} must both be [B,H,W]")
        B, H, W = lab.shape
        p = LgParams.from_buffer_copy(self._sync_params(image_processor))   # the selector's own params stay label-blind
        p.mask_is_bool = 1
        p.label_aware = 1 if label_aware else 0
        ids = (C.c_int32 * B)(*[(-(1 << 30)) if i is None else int(i) for i in leaf_ids])
        res = (LgGraspResult * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_select_grasp_labels(self._h, d.data_ptr(), lab.data_ptr(), ids, B, H, W, C.byref(p), None, None, res,
                                                      self._stream()), "lg_select_grasp_labels")
        for b, i in enumerate(leaf_ids):   # the node never calls select_grasp_point for a frame without a leaf (:113-116)
            if i is None:
                res[b].found = 0
        self.last_results = res
        return _triples(res, B)

    # ------------------------------------------------------------------ every candidate, ranked (:205-236)
    def _candidate_params(self, image_processor, top_k, is_bool):
        top_k = int(top_k)
        if not 1 <= top_k <= 64:
            raise ValueError(f"top_k must be in [1, 64] (got {top_k})")
        p = LgParams.from_buffer_copy(self._sync_params(image_processor))   # the selector's own params keep their top_k
        p.top_k = top_k
        p.mask_is_bool = 1 if is_bool else 0
        return p

    def select_grasp_candidates_batch(self, leaf_masks, depth_tensors, image_processor=None, top_k=20):
        """select_grasp_points_batch plus every candidate of every frame, ranked by the reference's own selection applied again
        to what is left after each pick (lg_select_grasp_candidates).  Returns (triples, cands): triples as
        select_grasp_points_batch returns them; cands a [B, top_k] numpy array of GRASP_CANDIDATE_DTYPE in rank order (rank 0 is
        the triple's point), rows past a frame's candidate count with index -1.  Bad input raises."""
        m, d, is_bool = self._prep_inputs(leaf_masks, depth_tensors)
        B, H, W = m.shape
        p = self._candidate_params(image_processor, top_k, is_bool)
        res = (LgGraspResult * B)()
        rows = (LgGraspCandidate * (B * p.top_k))()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_select_grasp_candidates(self._h, d.data_ptr(), m.data_ptr(), B, H, W, C.byref(p), res, rows,
                                                          self._stream()), "lg_select_grasp_candidates")
        self.last_results = res
        return _triples(res, B), np.frombuffer(rows, dtype=GRASP_CANDIDATE_DTYPE).reshape(B, p.top_k)

    def select_grasp_candidates_for_leaves(self, label_tensors, leaf_ids, depth_tensors, image_processor=None, top_k=20,
                                           label_aware=False):
        """select_grasp_candidates_batch(label_tensors == leaf_ids[:, None, None], depth_tensors) through the labels entry point
        (as select_grasp_points_for_leaves; the mask counts as a torch.bool tensor).  A None leaf id gives the (None, None, None)
        triple and zero candidate rows."""
        lab = label_tensors
        if not (torch.is_tensor(lab) and lab.dtype == torch.int16 and lab.is_cuda and lab.dim() == 3 and lab.is_contiguous()):
            raise ValueError("label_tensors must be a contiguous [B,H,W] int16 tensor on the device")
        d = depth_tensors.to(self.device, torch.float32).contiguous()
        if d.shape != lab.shape:
            raise ValueError(f"labels {tuple(lab.shape)} and depth {tuple(d.shape)} must both be [B,H,W]")
        B, H, W = lab.shape
        p = self._candidate_params(image_processor, top_k, True)
        p.label_aware = 1 if label_aware else 0   # (as select_grasp_points_for_leaves; every ranked candidate's pre-grasp too)
        ids = (C.c_int32 * B)(*[(-(1 << 30)) if i is None else int(i) for i in leaf_ids])   # no label carries it: no candidates
        res = (LgGraspResult * B)()
        rows = (LgGraspCandidate * (B * p.top_k))()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_select_grasp_candidates_labels(self._h, d.data_ptr(), lab.data_ptr(), ids, B, H, W, C.byref(p),
                                                                 res, rows, self._stream()), "lg_select_grasp_candidates_labels")
        cands = np.frombuffer(rows, dtype=GRASP_CANDIDATE_DTYPE).reshape(B, p.top_k)
        for b, i in enumerate(leaf_ids):   # no select_grasp_point call for a frame without a leaf: no triple, no candidates
            if i is None:
                res[b].found = 0
                cands[b] = np.zeros((), GRASP_CANDIDATE_DTYPE)
                cands[b]["index"] = -1
        self.last_results = res
        return _triples(res, B), cands

    def select_grasp_candidates(self, leaf_mask, depth_tensor, image_processor=None, top_k=20):
        """Every candidate of one frame in rank order, as a list of dicts: the lg_grasp_candidate fields plus point_2d, point_3d
        and pre_grasp_point shaped like select_grasp_point's triple (a NaN ML field and a missing pre-grasp point are None).
        The values the reference logs for each candidate (:210-236) and the runner-up grasps.  Never raises: errors are logged
        and give []."""
        try:
            _, cands = self.select_grasp_candidates_batch(leaf_mask, depth_tensor, image_processor=image_processor, top_k=top_k)
            out = []
            for row in cands[0].tolist():
                r = dict(zip(GRASP_CANDIDATE_DTYPE.names, row))
                if r["index"] < 0:
                    break
                for k in _ML_FIELDS:
                    if math.isnan(r[k]):
                        r[k] = None
                if not r["has_pre"]:
                    r["pX"] = r["pY"] = r["pZ"] = None
                r["point_2d"] = (r["x"], r["y"])
                r["point_3d"] = (r["X"], r["Y"], r["Z"])
                r["pre_grasp_point"] = (r["pX"], r["pY"], r["pZ"]) if r["has_pre"] else None
                out.append(r)
            return out
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in grasp candidate ranking: {str(e)}")
            return []

    def select_grasp_point(self, leaf_mask, depth_tensor, image_processor=None, pcl_data=None):
        """Select optimal grasp point using combined traditional and ML approach (reference :184)."""
        try:
            res = self.select_grasp_points_batch(leaf_mask, depth_tensor, image_processor=image_processor)[0]
            if res[0] is None:
                logwarn("No valid candidate points found")
            elif pcl_data is not None:
                # get_3d_grasp_point's point-cloud branch reads self.width, which the class never defines (:164-178): the
                # reference raises there and ends in its logged None triple
                raise AttributeError("'GraspPointSelector' object has no attribute 'width'")
            return res
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in grasp point selection: {str(e)}")
            return None, None, None

    # ------------------------------------------------------------------ ML-only selection (:290-390, the commented-out form)
    @staticmethod
    def ml_sampling(mode="nth", target=100, stride=8, max_samples=None, chunk=0):
        """An lg_ml_sampling: mode 'nth' (every step-th leaf pixel, step = max(1, n // target): the reference's walk) or 'grid'
        (the leaf pixels with x % stride == 0 and y % stride == 0).  max_samples: rows of the sample table per frame, default
        2 * target - 1 for 'nth' (all it can produce) and 4096 for 'grid' (a frame with more grid pixels overflows alone)."""
        modes = {"nth": _lib.LG_ML_SAMPLE_NTH, "grid": _lib.LG_ML_SAMPLE_GRID}
        if mode not in modes:
            raise ValueError(f"sampling mode must be 'nth' or 'grid' (got {mode!r})")
        if max_samples is None:
            max_samples = max(1, 2 * int(target) - 1) if mode == "nth" else 4096
        return LgMlSampling(modes[mode], int(target), int(stride), int(max_samples), int(chunk))

    def ml_planes(self, form=0):
        """Inspection / experiments (lg_debug_ml_planes): where the ML-only gather finds its planes from the next call on -- 0 by
        the library's rule, 1 computed at every window (deferred), 2 stored once by the plane kernel.  Returns the form the last
        ML-only call took (0: none yet).  Same results either way."""
        last = C.c_int32()
        check(self._h, lib.lg_debug_ml_planes(self._h, int(form), C.byref(last)), "lg_debug_ml_planes")
        return int(last.value)

    def _ml_finish(self, call, B, sampling, return_samples):
        s = sampling if sampling is not None else self.ml_sampling()
        res = (LgGraspResult * B)()
        rows = np.zeros((B, s.max_samples), ML_SAMPLE_DTYPE) if return_samples else None
        counts = np.zeros(B, np.int32)
        with torch.cuda.device(self.device):
            call(C.byref(s), res, rows.ctypes.data if return_samples else None, counts.ctypes.data_as(C.POINTER(C.c_int32)))
        self.last_results = res
        return res, rows, counts

    def select_grasp_points_ml_batch(self, leaf_masks, depth_tensors, sampling=None, return_samples=False, image_processor=None):
        """The ML-only selection for B frames (lg_select_grasp_ml): the CNN over sampled leaf pixels, the best logit or the mask
        centroid.  sampling: ml_sampling(...), default the reference's every-step-th walk with target 100.  Returns the triples
        as select_grasp_points_batch does; with return_samples also a [B, max_samples] array of ML_SAMPLE_DTYPE (x, y, scored,
        logit, ml_score; unscored rows NaN, rows past a frame's samples zero) and the frames' sample counts (int32 [B]; a
        'grid' frame with more samples than max_samples: -(their number), and no triple).  Bad input raises."""
        m, d, is_bool = self._prep_inputs(leaf_masks, depth_tensors)
        B, H, W = m.shape
        p = LgParams.from_buffer_copy(self._sync_params(image_processor))
        p.mask_is_bool = 1 if is_bool else 0
        res, rows, counts = self._ml_finish(
            lambda s, r, rw, cn: check(self._h, lib.lg_select_grasp_ml(self._h, d.data_ptr(), m.data_ptr(), B, H, W, C.byref(p), s, r, rw,
                                                                       cn, self._stream()), "lg_select_grasp_ml"),
            B, sampling, return_samples)
        out = _triples(res, B)
        return (out, rows, counts) if return_samples else out

    def select_grasp_points_ml_for_leaves(self, label_tensors, leaf_ids, depth_tensors, sampling=None, return_samples=False,
                                          image_processor=None, label_aware=False):
        """select_grasp_points_ml_batch(label_tensors == leaf_ids[:, None, None], depth_tensors) through the labels entry
        (lg_select_grasp_ml_labels), as select_grasp_points_for_leaves: a None leaf id gives the (None, None, None) triple;
        label_aware=True lets channel 5 and the pre-grasp clearance see the other leaves."""
        lab = label_tensors
        if not (torch.is_tensor(lab) and lab.dtype == torch.int16 and lab.is_cuda and lab.dim() == 3 and lab.is_contiguous()):
            raise ValueError("label_tensors must be a contiguous [B,H,W] int16 tensor on the device")
        d = depth_tensors.to(self.device, torch.float32).contiguous()
        if d.shape != lab.shape:
            raise ValueError(f"labels {tuple(lab.shape)} and depth {tuple(d.shape)} must both be [B,H,W]")
        B, H, W = lab.shape
        p = LgParams.from_buffer_copy(self._sync_params(image_processor))
        p.mask_is_bool = 1
        p.label_aware = 1 if label_aware else 0
        ids = (C.c_int32 * B)(*[(-(1 << 30)) if i is None else int(i) for i in leaf_ids])
        res, rows, counts = self._ml_finish(
            lambda s, r, rw, cn: check(self._h, lib.lg_select_grasp_ml_labels(self._h, d.data_ptr(), lab.data_ptr(), ids, B, H, W,
                                                                              C.byref(p), s, r, rw, cn, self._stream()),
                                       "lg_select_grasp_ml_labels"),
            B, sampling, return_samples)
        for b, i in enumerate(leaf_ids):
            if i is None:
                res[b].found = 0
        out = _triples(res, B)
        return (out, rows, counts) if return_samples else out

    def select_grasp_point_ml(self, leaf_mask, depth_tensor, image_processor=None, pcl_data=None):
        """The reference's "grasp point based on only ML model" select_grasp_point (:290-390), reference signature.  Never raises:
        errors are logged and give (None, None, None); pcl_data as in select_grasp_point."""
        try:
            res = self.select_grasp_points_ml_batch(leaf_mask, depth_tensor, image_processor=image_processor)[0]
            if res[0] is None:
                logwarn("No grasp point found (empty mask)")
            elif pcl_data is not None:
                raise AttributeError("'GraspPointSelector' object has no attribute 'width'")   # (see select_grasp_point)
            return res
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in grasp point selection: {str(e)}")
            return None, None, None

    def ml_score_map(self, leaf_mask, depth_tensor, stride=8, image_processor=None, max_samples=65536):
        """The model's score as a map over one leaf: (map, samples) -- map a [H,W] float32 device tensor holding ml_score at
        every scored grid pixel (x % stride == 0, y % stride == 0, on the leaf, off the 16-pixel border band) and NaN elsewhere;
        samples the frame's rows of ML_SAMPLE_DTYPE.  A leaf with more grid pixels than max_samples raises."""
        s = self.ml_sampling("grid", stride=stride, max_samples=max_samples)
        _, rows, counts = self.select_grasp_points_ml_batch(leaf_mask, depth_tensor, sampling=s, return_samples=True,
                                                            image_processor=image_processor)
        if counts[0] < 0:
            raise ValueError(f"ml_score_map: {-int(counts[0])} grid pixels, more than max_samples = {max_samples}")
        rows = rows[0, :int(counts[0])]
        H, W = (leaf_mask.shape[-2], leaf_mask.shape[-1])
        out = torch.full((H, W), float("nan"), dtype=torch.float32, device=self.device)
        sc = rows[rows["scored"] != 0]
        if len(sc):
            yi = torch.from_numpy(sc["y"].astype(np.int64)).to(self.device)
            xi = torch.from_numpy(sc["x"].astype(np.int64)).to(self.device)
            out[yi, xi] = torch.from_numpy(np.ascontiguousarray(sc["ml_score"])).to(self.device)
        return out, rows

    # ------------------------------------------------------------------ small host-side helpers kept for callers
    def get_3d_grasp_point(self, grasp_point_2d, depth_tensor, pcl_data=None):  # :152-180
        u, v = grasp_point_2d
        depth_value = depth_tensor[v, u].item()
        return ((depth_value * (u - self.camera_cx)) / self.f_norm,
                (depth_value * (v - self.camera_cy)) / self.f_norm, depth_value)

    def _project_point_to_2d(self, point_3d):  # :821-826
        x, y, z = point_3d
        return (int((x * self.f_norm / z) + self.camera_cx), int((y * self.f_norm / z) + self.camera_cy))

    def estimate_leaf_orientation(self, leaf_mask_np):  # :718-752 (LeafVisualizer calls this, visualizer.py:77)
        """(angle_rad, major_axis, minor_axis, (cx, cy)) or four Nones."""
        try:
            m = torch.as_tensor(np.asarray(leaf_mask_np) if not torch.is_tensor(leaf_mask_np) else leaf_mask_np)
            m = (m.to(self.device) != 0).to(torch.uint8).contiguous()
            H, W = m.shape
            out = (C.c_float * 5)()
            found = C.c_int(0)
            with torch.cuda.device(self.device):
                check(self._h, lib.lg_leaf_orientation(self._h, m.data_ptr(), H, W, out, C.byref(found),
                                                       self._stream()), "lg_leaf_orientation")
            if not found.value:
                return None, None, None, None
            return float(out[0]), float(out[1]), float(out[2]), (float(out[3]), float(out[4]))
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in leaf orientation estimation: {str(e)}")
            return None, None, None, None

    # ------------------------------------------------------------------ midrib (:829-922; LeafVisualizer calls it, visualizer.py:141)
    def _prep_midrib(self, leaf_masks, raw_images):
        m = leaf_masks if torch.is_tensor(leaf_masks) else torch.from_numpy(np.ascontiguousarray(leaf_masks))
        im = raw_images if torch.is_tensor(raw_images) else torch.from_numpy(np.ascontiguousarray(raw_images))
        if im.dtype != torch.uint8:
            raise ValueError(f"image must be uint8 (got {im.dtype})")
        if m.dim() != 3 or im.dim() != 4 or tuple(im.shape[:3]) != tuple(m.shape) or im.shape[3] not in (3, 4):
            raise ValueError(f"mask {tuple(m.shape)} and image {tuple(im.shape)} must be [B,H,W] and [B,H,W,C] with C 3 or 4")
        m = m.to(self.device).contiguous()
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)   # one 0/1 byte per element: reinterpret, no kernel
        elif m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
        return m.contiguous(), im.to(self.device).contiguous()

    def detect_midrib_batch(self, leaf_masks, raw_images):
        """detect_midrib of B frames in one library call: leaf_masks [B,H,W] (u8 / bool, nonzero = leaf), raw_images [B,H,W,C]
        uint8 with C 3 or 4, numpy or tensors.  Returns a list of B results, each ((x0, y0), (x1, y1)) of Python ints or None.
        Bad input raises; the per-frame status words stay in `last_midrib_status`."""
        m, im = self._prep_midrib(leaf_masks, raw_images)
        B, H, W = m.shape
        out, st = (C.c_int32 * (4 * B))(), (C.c_int32 * B)()
        with torch.cuda.device(self.device):
            check(self._h, lib.lg_detect_midrib(self._h, im.data_ptr(), int(im.shape[3]), m.data_ptr(), B, H, W, out, st,
                                                self._stream()), "lg_detect_midrib")
        res = []
        for b in range(B):
            if st[b] == MIDRIB_FOUND:
                res.append(((out[4 * b], out[4 * b + 1]), (out[4 * b + 2], out[4 * b + 3])))
            else:
                if st[b] == MIDRIB_THIN:   # the reference's cv2.line(..., thickness=int(minor/6)) asserts: logged, None
                    logerr("Error in midrib detection: line thickness int(minor_axis / 6) is 0 (minor axis < 6)")
                res.append(None)
        self.last_midrib_status = list(st)
        return res

    def detect_midrib(self, leaf_mask_np, raw_image):
        """Reference signature (:829): ((x0, y0), (x1, y1)) of the detected ridge's first and last point, or None.
        leaf_mask_np: [H,W] u8 / bool (numpy or tensor); raw_image: [H,W,C] uint8 (numpy or device tensor), C 3 or 4, channels
        weighted by index as cv2's BGR2GRAY does.  Never raises: errors are logged and give None."""
        try:
            m = leaf_mask_np if torch.is_tensor(leaf_mask_np) else torch.from_numpy(np.ascontiguousarray(leaf_mask_np))
            im = raw_image if torch.is_tensor(raw_image) else torch.from_numpy(np.ascontiguousarray(raw_image))
            if m.dim() != 2 or im.dim() != 3:
                raise ValueError(f"mask {tuple(m.shape)} and image {tuple(im.shape)} must be [H,W] and [H,W,C]")
            return self.detect_midrib_batch(m.unsqueeze(0), im.unsqueeze(0))[0]
        except Exception as e:  # noqa: BLE001
            logerr(f"Error in midrib detection: {str(e)}")
            return None


def _triples(res, B):
    """(xy, XYZ, preXYZ) triples of B lg_grasp_result rows.  One structured view of the rows instead of a ctypes attribute access
    per field and frame (0.12 -> 0.04 ms per 256 frames; float32 -> Python float conversions are the same values either way)."""
    a = np.frombuffer(res, dtype=_RESULT_DTYPE, count=B)
    cols = [a[n].tolist() for n in ("found", "x", "y", "X", "Y", "Z", "has_pre", "pX", "pY", "pZ")]
    return [((x, y), (X, Y, Z), (pX, pY, pZ) if hp else None) if f else (None, None, None)
            for f, x, y, X, Y, Z, hp, pX, pY, pZ in zip(*cols)]


_clahe_handles = {}   # device index -> (lock, handle) of leafgrasp_amd.clahe
_clahe_lock = threading.Lock()


def clahe(gray, clip_limit=3.0, tile_grid_size=(8, 8)):
    """cv2.createCLAHE(clipLimit=clip_limit, tileGridSize=tile_grid_size).apply(gray) on the device (lg_clahe).
    gray: uint8 tensor [H,W] or [B,H,W] (a CPU tensor or numpy array is moved to the current device); returns a uint8 device
    tensor of the same shape.  tile_grid_size is (tiles across, tiles down), as OpenCV takes it."""
    g = gray if torch.is_tensor(gray) else torch.from_numpy(np.ascontiguousarray(gray))
    if g.dtype != torch.uint8 or g.dim() not in (2, 3):
        raise ValueError(f"clahe needs a uint8 [H,W] or [B,H,W] image (got {g.dtype} {tuple(g.shape)})")
    dev = g.device if g.is_cuda else torch.device("cuda", torch.cuda.current_device())
    idx = _device_index(dev)
    x = g.to(dev).contiguous()
    x3 = x.unsqueeze(0) if x.dim() == 2 else x
    B, H, W = x3.shape
    out = torch.empty_like(x3)
    tx, ty = (int(v) for v in tile_grid_size)
    with _clahe_lock:
        if idx not in _clahe_handles:
            h = _VP()
            check(None, lib.lg_create(idx, C.byref(h)), "lg_create")
            _clahe_handles[idx] = (threading.Lock(), h)
        lock, h = _clahe_handles[idx]
    with lock, torch.cuda.device(dev):
        check(h, lib.lg_clahe(h, x3.data_ptr(), B, H, W, float(clip_limit), tx, ty, out.data_ptr(),
                              _VP(torch.cuda.current_stream(dev).cuda_stream)), "lg_clahe")
    return out[0] if x.dim() == 2 else out
