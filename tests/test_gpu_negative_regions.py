"""lg_negative_masks and lg_leaf_contour against the oracle at frame shapes that exercise the kernels' guards (-m gpu).

Whole tip and stem planes, not only the point lists, against a full-plane NumPy restatement (tests/collector_cases.py:
tip_plane, stem_plane; held to the oracle's collector_tip_points / collector_stem_points in tests/test_collector_edges.py)
and the mirror methods _get_tip_points / _get_stem_points / _get_edge_points against the oracle's lists.  Shapes: narrower
than one 64-column tile, one column past it, H no multiple of the 4-row tile, 0.75 H fractional.  Masks: plateaus, leaves
on the bottom row and the sides (cv2's morphology ignores the border), bars that two erosions remove or thin to a line,
a rectangle whose top-quarter cut falls inside a run of equal distances.  Everything is compared bit for bit.  cv2 itself
is on neither side: this pins the product to the ORACLE's restatement of distanceTransform / erode / findContours."""
import ctypes as C

import numpy as np
import pytest

from oracle import lg_oracle as O
from tests import collector_cases as CC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REGION_SHAPES = [(5, 7), (33, 47), (63, 65), (67, 130), (160, 224)]
CONTOUR_SHAPES = [(33, 47), (64, 96), (67, 130)]


@pytest.fixture(scope="module")
def collector(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import leafgrasp_amd as L

    return L.EnhancedGraspDataCollector(patch_size=32, resume=False, data_dir=str(tmp_path_factory.mktemp("lg_regions")),
                                        device="cuda:0")


def _negative_planes(col, mask, dist):
    """lg_negative_masks through the C-ABI on sentinel-filled planes: every pixel must be written, with 0 or 1."""
    from leafgrasp_amd._lib import check, lib

    H, W = mask.shape
    m = torch.from_numpy(mask).to(col.device)
    d = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32)).to(col.device)
    tip = torch.full((H, W), 7, dtype=torch.uint8, device=col.device)
    stem = torch.full((H, W), 7, dtype=torch.uint8, device=col.device)
    with torch.cuda.device(col.device):
        check(col._h, lib.lg_negative_masks(col._h, d.data_ptr(), m.data_ptr(), H, W, tip.data_ptr(), stem.data_ptr(),
                                            col._stream()), "lg_negative_masks")
        torch.cuda.synchronize()
    return tip.cpu().numpy(), stem.cpu().numpy()


def _points(plane):
    ys, xs = np.nonzero(plane)
    return list(zip(xs.tolist(), ys.tolist()))


@pytest.mark.parametrize("shape", REGION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_negative_planes_and_point_lists_vs_oracle(collector, shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    seen_tie = False
    for name, m in CC.region_masks(H, W).items():
        dist = O.distance_transform(m, 5)
        tip, stem = _negative_planes(collector, m, dist)
        np.testing.assert_array_equal(tip, CC.tip_plane(m, dist), err_msg=f"tip plane {name}")
        np.testing.assert_array_equal(stem, CC.stem_plane(m), err_msg=f"stem plane {name}")
        # the planes carry the oracle's lists: stem in row-major order, tip sorted by distance (stable), top quarter
        assert _points(stem) == O.collector_stem_points(m), name
        allp = _points(tip)
        allp.sort(key=lambda p: dist[p[1], p[0]], reverse=True)
        assert (allp[:max(1, len(allp) // 4)] if allp else []) == O.collector_tip_points(m), name
        cut = max(1, len(allp) // 4)
        seen_tie |= len(allp) > cut and dist[allp[cut - 1][1], allp[cut - 1][0]] == dist[allp[cut][1], allp[cut][0]]
        # a plane that is no transform of this mask: small integers, so 5x5 ties are everywhere
        other = rng.integers(0, 4, (H, W)).astype(np.float32)
        tip2, stem2 = _negative_planes(collector, m, other)
        np.testing.assert_array_equal(tip2, CC.tip_plane(m, other), err_msg=f"tip plane {name}, foreign plane")
        np.testing.assert_array_equal(stem2, stem, err_msg=f"stem plane {name}: independent of the distance plane")
        # the mirror methods.  lg_score_maps, which computes the transform on the device, takes frames from 8x8 up:
        # below that the transform is handed in
        mt = torch.from_numpy(m).to(collector.device)
        got_tip = collector._get_tip_points(mt) if min(H, W) >= 8 else collector._get_tip_points(mt, torch.from_numpy(dist))
        assert got_tip == O.collector_tip_points(m), f"_get_tip_points {name}"
        assert collector._get_stem_points(mt) == O.collector_stem_points(m), f"_get_stem_points {name}"
        assert collector._get_edge_points(mt) == O.collector_edge_points(m), f"_get_edge_points {name}"
    assert seen_tie                                       # the stable row-major order decided at least one cut
    masks = CC.region_masks(H, W)
    if W >= 11 and H - int(0.75 * H) >= 5:                # (the 5x7 frame has no room for the bars)
        assert O.collector_stem_points(masks["bar5"]) == []
        assert len({x for x, _ in O.collector_stem_points(masks["bar9"])}) == 1
        ridge = masks["ridge"]
        dist = O.distance_transform(ridge, 5)
        allp = _points(CC.tip_plane(ridge, dist))
        allp.sort(key=lambda p: dist[p[1], p[0]], reverse=True)
        cut = max(1, len(allp) // 4)
        assert dist[allp[cut - 1][1], allp[cut - 1][0]] == dist[allp[cut][1], allp[cut][0]]


def _contour(col, mask, cap, buf):
    from leafgrasp_amd._lib import check, lib

    H, W = mask.shape
    m = torch.from_numpy(mask).to(col.device)
    n = C.c_int(-1)
    with torch.cuda.device(col.device):
        check(col._h, lib.lg_leaf_contour(col._h, m.data_ptr(), H, W, buf.ctypes.data if buf is not None else None, cap,
                                          C.byref(n), col._stream()), "lg_leaf_contour")
    return n.value


@pytest.mark.parametrize("shape", CONTOUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_leaf_contour_and_edge_points_vs_oracle(collector, shape):
    H, W = shape
    masks = CC.contour_masks(H, W)
    first_cap = 4 * (H + W) + 16
    if shape == (64, 96):
        assert len(O.leaf_contour_points(masks["comb"])) > first_cap      # _get_edge_points has to ask again
    for name, m in masks.items():
        exp = O.leaf_contour_points(m)
        n = len(exp)
        buf = np.full((n + 4, 2), -7, np.int32)
        assert _contour(collector, m, n + 4, buf) == n, name
        np.testing.assert_array_equal(buf[:n], exp, err_msg=name)
        assert (buf[n:] == -7).all(), name
        # cap = 0: the count alone; cap = n - 1: n - 1 points, nothing behind them
        assert _contour(collector, m, 0, None) == n, name
        if n >= 1:
            buf = np.full((n + 4, 2), -7, np.int32)
            assert _contour(collector, m, n - 1, buf) == n, name
            np.testing.assert_array_equal(buf[:n - 1], exp[:n - 1], err_msg=name)
            assert (buf[n - 1:] == -7).all(), name
        mt = torch.from_numpy(m).to(collector.device)
        assert collector._get_edge_points(mt) == O.collector_edge_points(m), f"_get_edge_points {name}"
    assert O.collector_edge_points(masks["comb"]) and O.collector_edge_points(masks["line"])
