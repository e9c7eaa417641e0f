"""Test-side reference of the label-aware mode (lg_params.label_aware = 1), composed from the oracle's parts: the isolation map
of grasp_point_selector.py:595-633 with `other_leaves` taken from the label image, and calculate_pre_grasp_point (:754-819)
probing every leaf.  RefGraspPointSelector itself is not edited: LabelAwareRef subclasses it."""
import numpy as np

from oracle import lg_oracle as O


def split(labels, leaf_id):
    """current, others, all as uint8 images: a label <= 0 is background"""
    labels = np.asarray(labels)
    cur = (labels == leaf_id).astype(np.uint8)
    oth = ((labels > 0) & (labels != leaf_id)).astype(np.uint8)
    return cur, oth, (labels > 0).astype(np.uint8)


def transforms(others, init_dist0=O.INIT_DIST0):
    """(dc, dw) float32 and (dc_fix, dw_fix) uint32 of an image with another leaf: oracle lines 399-403"""
    out = []
    for k in (30, 40):
        dil = O.dilate(others, O.ellipse_se(k))
        out.append(O.distance_transform(1 - dil, 3, return_fix=True, init_dist0=init_dist0))
    (dc, dcf), (dw, dwf) = out
    return (dc, dw), (dcf, dwf)


def isolation_plane(labels, leaf_id, params=None):
    """_calculate_isolation_score (oracle lines 394-408) with `other` = the other leaves of the label image"""
    p = O.ref_params(params)
    cur, oth, _ = split(labels, leaf_id)
    height, width = cur.shape
    ic = O.dilate(oth, O.ellipse_se(30))
    dc = O.distance_transform(1 - ic, 3, init_dist0=p.chamfer_init_dist0)
    sc = dc / (np.max(dc) + 1e-6)
    iw = O.dilate(oth, O.ellipse_se(40))
    dw = O.distance_transform(1 - iw, 3, init_dist0=p.chamfer_init_dist0)
    sw = dw / (np.max(dw) + 1e-6)
    iso = (p.iso_w_close * sc + p.iso_w_wide * sw).astype(np.float32)
    yc = np.linspace(p.iso_ramp_top, p.iso_ramp_bottom, height)[:, np.newaxis]
    hp = np.tile(yc, (1, width))
    return iso * hp * cur


class LabelAwareRef(O.RefGraspPointSelector):
    """select_grasp_point of one leaf of a label image with both label-aware substitutions"""

    def __init__(self, labels, leaf_id, **kw):
        super().__init__(**kw)
        self.labels = np.asarray(labels)
        self.leaf_id = leaf_id
        self.current, self.others, self.all = split(labels, leaf_id)

    def _calculate_isolation_score(self, m):
        return isolation_plane(self.labels, self.leaf_id, self.params)

    def calculate_pre_grasp_point(self, g3, m):
        return super().calculate_pre_grasp_point(g3, self.all)

    def select(self, depth_f32, **kw):
        return self.select_grasp_point(self.current, depth_f32, **kw)


def blob_labels(H, W, blobs):
    """label image from ellipses (id, cx, cy, rx, ry), later blobs on top (synthetic_inputs-style leaves)"""
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((H, W), np.int16)
    for i, cx, cy, rx, ry in blobs:
        lab[((xx - cx) / float(rx)) ** 2 + ((yy - cy) / float(ry)) ** 2 <= 1.0] = i
    return lab
