"""GPU parity of the leaf-selection stage (OptimalLeafSelector), the ROS-free node harness and the
HybridGraspSelector facade against the CPU oracle."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


@pytest.mark.parametrize("shape,seed", [((270, 360), 0), ((360, 480), 1), ((720, 1280), 2), ((1080, 1440), 3),
                                        ((1080, 1920), 4), ((300, 517), 5)])
def test_leaf_statistics_and_selection(L, shape, seed):
    H, W = shape
    labels, depth, P = O.synthetic_scene(H, W, seed)
    ols = L.OptimalLeafSelector("cuda:0")
    ols.set_camera_params(P)
    stats, (mn, mx), _ = ols.leaf_statistics(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())
    ids = np.unique(labels)
    ids = ids[ids > 0]
    assert [s["id"] for s in stats] == ids.tolist()
    for s in stats:                                     # integer / order statistics: bit-exact
        lm = labels == s["id"]
        ys, xs = np.where(lm)
        assert s["area"] == int(lm.sum())
        assert s["sum_x"] == float(xs.sum()) and s["sum_y"] == float(ys.sum())
        assert s["touches_border"] == bool(lm[0].any() or lm[-1].any() or lm[:, 0].any() or lm[:, -1].any())
        assert s["median_depth"] == np.median(depth[lm])
        assert s["sum_depth"] == pytest.approx(float(depth[lm].astype(np.float64).sum()), rel=1e-12)
        ray = np.sqrt((xs - P[0, 2]) ** 2 + (ys - P[1, 2]) ** 2 + P[0, 0] ** 2).sum()
        assert s["sum_ray"] == pytest.approx(ray, rel=1e-6)   # camera constants travel as float32
    emn, emx = O.clutter_extrema(labels)
    assert mn == tuple(int(v) for v in emn)
    assert mx == tuple(int(v) for v in emx)
    ref = O.RefOptimalLeafSelector()
    ref.set_camera_params(P)
    r = ref.select_optimal_leaf(labels, depth, return_debug=True)
    g = ols.select_optimal_leaf(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda(), return_debug=True)
    if r is None:   # no leaf reaches the 10000 px floor at this size (leaf_scorer.py:79-81)
        assert g is None
        return
    (exp, dbg), (got, gdbg) = r, g
    assert got == exp
    assert ols.get_tall_leaves() == ref.get_tall_leaves()
    for a, b in zip(gdbg["candidates"], dbg["candidates"]):
        assert a["leaf_id"] == b["leaf_id"]
        np.testing.assert_allclose(a["scores"], b["scores"], rtol=1e-4, atol=1e-7)


# Measured bound of the one deliberate semantic substitution on this path: the HIP clutter
# field is the EXACT Euclidean distance, the reference's is skfmm's second-order fast-marching approximation
# (leaf_scorer.py:66-71), restated in oracle/lg_oracle.c::lg_fmm_distance.  Over 120 scenes (40 seeds x 720p / native /
# 1080p, /tmp sweep of round 2): arg-max moved by <= 1 px, |d clutter_score| <= 2.7e-4, 0 different leaf ids, 0 different
# tall-leaf lists; on the HIP path in these 36 scenes: 1 px, 2.8e-4 absolute on scores of 0.3-0.7, i.e. up to ~5e-4 RELATIVE --
# above north_star's 1e-4 float bar: this is the documented deviation of the substitution, not rounding.  The bounds asserted
# are the measured values plus a margin (1 px is the grid; 4e-4 = 1.4 x measured).
_FMM_ARGMAX_PX = 1.0
_FMM_CLUTTER_ABS = 4e-4


@pytest.mark.parametrize("shape", [(720, 1280), (1080, 1440), (1080, 1920)])
def test_hip_clutter_extrema_vs_restated_fmm(L, shape):
    H, W = shape
    ols = L.OptimalLeafSelector("cuda:0")
    worst_px, worst_cl, n_sel = 0.0, 0.0, 0
    for seed in range(40, 52):
        labels, depth, P = O.synthetic_scene(H, W, seed)
        ols.set_camera_params(P)
        g = ols.select_optimal_leaf(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda(), return_debug=True)
        ref = O.RefOptimalLeafSelector("fmm")          # the reference's field semantics
        ref.set_camera_params(P)
        r = ref.select_optimal_leaf(labels, depth, return_debug=True)
        if r is None:
            assert g is None
            continue
        (exp, dbg), (got, gdbg) = r, g
        (gmn, gmx), (fmn, fmx) = gdbg["extrema"], dbg["extrema"]
        assert tuple(gmn) == tuple(int(v) for v in fmn)                 # first leaf pixel either way
        worst_px = max(worst_px, float(np.hypot(gmx[0] - fmx[0], gmx[1] - fmx[1])))
        assert [c["leaf_id"] for c in gdbg["candidates"]] == [c["leaf_id"] for c in dbg["candidates"]]
        for a, b in zip(gdbg["candidates"], dbg["candidates"]):
            worst_cl = max(worst_cl, abs(a["scores"][0] - b["scores"][0]))
            np.testing.assert_allclose(a["scores"][1:], b["scores"][1:], rtol=1e-4, atol=1e-7)   # distance, visibility
        assert got == exp, f"seed {seed}: HIP (EDT) picks leaf {got}, restated FMM semantics pick {exp}"
        assert ols.get_tall_leaves() == ref.get_tall_leaves()
        n_sel += 1
    assert n_sel >= 8
    assert worst_px <= _FMM_ARGMAX_PX, worst_px
    assert worst_cl <= _FMM_CLUTTER_ABS, worst_cl


def test_leaf_many_labels(L):
    """leaf_scorer.py:32 takes any number of labels (torch.unique).  The LDS histograms of the median pass hold 64 slots; frames
    with more labels run further slot groups (up to 1024 labels): statistics and medians stay exact, the wrapper re-reads the
    frame with room for the results."""
    rng = np.random.default_rng(5)
    H, W = 360, 480
    labels = np.zeros((H, W), np.int16)
    ids = rng.permutation(np.arange(1, 30000))[:330]
    k = 0
    for by in range(15):
        for bx in range(22):
            labels[4 + by * 23: 4 + by * 23 + 17 + (k % 5), 3 + bx * 21: 3 + bx * 21 + 16 + (k % 3)] = ids[k]
            k += 1
    depth = (0.4 + 0.2 * rng.random((H, W))).astype(np.float32)
    depth[::7, ::5] = 0.5                                        # repeated values: duplicates around the median
    ols = L.OptimalLeafSelector("cuda:0")
    ols.set_camera_params(np.array([[500.0, 0, 240, -20], [0, 500, 180, 0], [0, 0, 1, 0]]))
    stats, (mn, mx), _ = ols.leaf_statistics(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())
    uniq = np.unique(labels)
    uniq = uniq[uniq > 0]
    assert len(uniq) == 330 and [s["id"] for s in stats] == uniq.tolist()
    for s in stats[::7] + stats[-3:]:
        lm = labels == s["id"]
        ys, xs = np.where(lm)
        assert s["area"] == int(lm.sum()) and s["sum_x"] == float(xs.sum()) and s["sum_y"] == float(ys.sum())
        assert s["median_depth"] == np.median(depth[lm])
        assert s["sum_depth"] == pytest.approx(float(depth[lm].astype(np.float64).sum()), rel=1e-12)
    emn, emx = O.clutter_extrema(labels)
    assert mn == tuple(int(v) for v in emn) and mx == tuple(int(v) for v in emx)
    # the batched entry point: one frame with many labels beside ordinary ones
    lab2, dep2, _ = O.synthetic_scene(H, W, 3)
    out = ols.leaf_statistics_batch(torch.from_numpy(np.stack([lab2, labels, lab2])).cuda(),
                                    torch.from_numpy(np.stack([dep2, depth, dep2])).cuda())
    assert [s["id"] for s in out[1][0]] == uniq.tolist()
    assert len(out[0][0]) == len(np.unique(lab2)) - 1
    for a, b in zip(out[0][0], out[2][0]):   # (float sums are accumulated with atomics: equal to the last bit or two, not bitwise)
        assert (a["id"], a["area"], a["sum_x"], a["sum_y"], a["median_depth"]) == (b["id"], b["area"], b["sum_x"], b["sum_y"], b["median_depth"])
    for a, b in zip(out[1][0], stats):
        assert a["area"] == b["area"] and a["median_depth"] == b["median_depth"]
    # more than 1024 labels: that frame alone is refused (None), logged, never raised
    many = np.zeros((H, W), np.int16)
    many.reshape(-1)[:1100 * 3:3] = np.arange(1, 1101)
    out = ols.leaf_statistics_batch(torch.from_numpy(np.stack([lab2, many])).cuda(), torch.from_numpy(np.stack([dep2, depth])).cuda())
    assert out[0] is not None and out[1] is None
    assert ols.select_optimal_leaf(torch.from_numpy(many).cuda(), torch.from_numpy(depth).cuda()) is None
    # the native batched selection (lg_leaf_select_batch): a frame with >= 128 labels (numpy's summation order of the mean of
    # medians changes there) or with more rows than the entry point reads back (330) takes the per-frame path, 1100 labels give
    # None; the ordinary frames beside them are unaffected
    lab3, dep3, _ = O.synthetic_scene(540, 720, 41)               # leaves above the 10000 px area threshold
    crowded = lab3.copy()
    k = 0
    for y in range(2, 538, 12):
        for x in range(2, 718, 12):
            if k < 140 and not lab3[y:y + 3, x:x + 3].any():
                crowded[y:y + 3, x:x + 3] = 1000 + k
                k += 1
    assert k == 140
    grid = np.zeros((540, 720), np.int16); grid[:H, :W] = labels
    many2 = np.zeros((540, 720), np.int16); many2[:H, :W] = many
    dgrid = np.full((540, 720), 0.5, np.float32); dgrid[:H, :W] = depth
    lab_b = torch.from_numpy(np.stack([lab3, crowded, grid, many2])).cuda()
    dep_b = torch.from_numpy(np.stack([dep3, dep3, dgrid, dgrid])).cuda()
    got = ols.select_optimal_leaves_batch(lab_b, dep_b)
    want = [ols.select_optimal_leaf(lab_b[b], dep_b[b]) for b in range(4)]
    assert got == want and got[0] is not None and got[1] is not None and got[3] is None
    ref = O.RefOptimalLeafSelector()
    ref.set_camera_params(np.array([[500.0, 0, 240, -20], [0, 500, 180, 0], [0, 0, 1, 0]]))
    assert got[1] == ref.select_optimal_leaf(crowded, dep3)


def test_clutter_argmax_branch_and_bound_adversarial(L):
    """The arg-max of the exact distance field comes from a branch-and-bound pass on the leaf bit mask (lg_leaf.hip::k_edt_bb):
    ties (first occurrence in row-major order), single pixels, lines, frames without / full of leaves, widths that are not a
    multiple of 64 -- always the oracle's np.argmax of the exact field."""
    from scipy import ndimage

    rng = np.random.default_rng(9)
    ols = L.OptimalLeafSelector("cuda:0")
    ols.set_camera_params(np.array([[500.0, 0, 240, -20], [0, 500, 180, 0], [0, 0, 1, 0]]))
    cases = []
    for (H, W) in ((64, 64), (97, 133), (300, 517), (720, 1280)):
        z = np.zeros((H, W), np.int16)
        a = z.copy(); a[0, 0] = 1; cases.append(a)                              # far corner wins
        a = z.copy(); a[H // 2, W // 2] = 2; cases.append(a)                    # four corners tie -> (0, 0)... or the nearest tie
        a = z.copy(); a[H // 2, :] = 1; cases.append(a)                         # line: whole top / bottom rows tie
        a = z.copy(); a[:, W // 3] = 3; cases.append(a)
        a = z.copy(); a[0, 0] = a[H - 1, W - 1] = a[0, W - 1] = a[H - 1, 0] = 1; cases.append(a)   # centre region
        a = np.ones((H, W), np.int16); a[H // 3, W // 5] = 0; cases.append(a)   # one background pixel
        a = z.copy(); a[rng.random((H, W)) > 0.999] = 4; cases.append(a)        # sparse specks
        a = z.copy(); a[::16, ::16] = 5; cases.append(a)                        # lattice: many equal maxima
        a = (rng.random((H, W)) > 0.5).astype(np.int16); cases.append(a)        # dense noise: maxima of a few pixels
        cases.append(np.ones((H, W), np.int16))                                 # no background pixel
    for i, lab in enumerate(cases):
        d = np.full(lab.shape, 0.5, np.float32)
        _, (mn, mx), _ = ols.leaf_statistics(torch.from_numpy(lab).cuda(), torch.from_numpy(d).cuda())
        leaf = lab >= 1
        e = ndimage.distance_transform_edt(~leaf)
        emx = np.unravel_index(e.argmax(), e.shape)
        assert mx == tuple(int(v) for v in emx), f"case {i} {lab.shape}: {mx} vs {emx} (d2 {e[mx] ** 2} vs {e[emx] ** 2})"
        emn = np.unravel_index(e.argmin(), e.shape)
        assert mn == tuple(int(v) for v in emn), f"case {i}"
    empty = np.zeros((100, 130), np.int16)
    _, (mn, mx), _ = ols.leaf_statistics(torch.from_numpy(empty).cuda(), torch.from_numpy(np.zeros((100, 130), np.float32)).cuda())
    assert mn == (0, 0) and mx == (0, 0)


def test_leaf_selection_edge_cases(L):
    ols = L.OptimalLeafSelector("cuda:0")
    P = np.array([[300.0, 0, 100, -20], [0, 300, 80, 0], [0, 0, 1, 0]])
    ols.set_camera_params(P)
    H, W = 160, 200
    depth = np.full((H, W), 0.5, np.float32)
    empty = np.zeros((H, W), np.int16)
    assert ols.select_optimal_leaf(torch.from_numpy(empty).cuda(), torch.from_numpy(depth).cuda()) is None
    small = empty.copy()
    small[10:20, 10:20] = 3                                   # area < 10000 -> no candidate
    assert ols.select_optimal_leaf(torch.from_numpy(small).cuda(), torch.from_numpy(depth).cuda()) is None
    big = empty.copy()
    big[20:140, 30:170] = 7                                   # one interior leaf, even pixel count, constant depth
    big[0:5, 0:5] = 2
    ref = O.RefOptimalLeafSelector()
    ref.set_camera_params(P)
    assert ols.select_optimal_leaf(torch.from_numpy(big).cuda(), torch.from_numpy(depth).cuda()) == \
        ref.select_optimal_leaf(big, depth) == 7
    # even count with two distinct middle values: float32 mean of the two
    d2 = depth.copy()
    d2[20:80, 30:170] = 0.25
    stats, _, _ = ols.leaf_statistics(torch.from_numpy(big).cuda(), torch.from_numpy(d2).cuda())
    s7 = [s for s in stats if s["id"] == 7][0]
    assert s7["median_depth"] == np.median(d2[big == 7]) == np.float32(0.375)


def test_estimate_leaf_orientation(L):
    sel = L.GraspPointSelector("cuda:0", load_model=False)
    for seed in (0, 1, 2):
        labels, _, _ = O.synthetic_scene(270, 360, seed)
        m = (labels == 1).astype(np.uint8)
        got = sel.estimate_leaf_orientation(m)
        exp = O.RefGraspPointSelector().estimate_leaf_orientation(m)
        assert got[0] == pytest.approx(exp[0], abs=1e-6)
        assert got[1] == pytest.approx(exp[1], rel=1e-5) and got[2] == pytest.approx(exp[2], rel=1e-5)
        assert got[3] == pytest.approx(exp[3], rel=1e-5)
    assert sel.estimate_leaf_orientation(np.zeros((64, 64), np.uint8)) == (None, None, None, None)


def _orientation_cases():
    """Masks for the contour analysis: the shapes of tests/test_host_contour.py (noise, sparse specks, an ellipse with a hole
    and a fragment, full frames, ragged bands) plus leaf-like scenes with several components, thin bridges and spirals."""
    rng = np.random.default_rng(11)
    cases = []
    for case in range(120):
        H, W = int(rng.integers(3, 90)), int(rng.integers(3, 200))
        kind = case % 6
        yy, xx = np.mgrid[0:H, 0:W]
        if kind == 0:
            m = rng.random((H, W)) > 0.6
        elif kind == 1:
            m = rng.random((H, W)) > 0.97
        elif kind == 2:
            m = ((xx - W * 0.5) / (W * 0.4)) ** 2 + ((yy - H * 0.5) / (H * 0.35)) ** 2 <= 1
            m &= ~(((xx - W * 0.5) / (W * 0.15)) ** 2 + ((yy - H * 0.5) / (H * 0.12)) ** 2 <= 1)   # a hole
            m[0, :3] = True
        elif kind == 3:
            m = np.ones((H, W), bool)
        elif kind == 4:
            m = np.zeros((H, W), bool)
            h4 = min(max(1, H // 4), H - H // 3)
            m[H // 3: H // 3 + h4, :] = rng.random((h4, W)) > 0.3
        else:   # a rotated bar and a diagonal one-pixel line joined to it (the border passes the line's pixels twice)
            a = rng.uniform(0, np.pi)
            u = (xx - W / 2) * np.cos(a) + (yy - H / 2) * np.sin(a)
            v = -(xx - W / 2) * np.sin(a) + (yy - H / 2) * np.cos(a)
            m = (np.abs(u) < W * 0.3) & (np.abs(v) < max(1.5, H * 0.08))
            k = np.arange(min(H, W))
            m[k, k] = True
        cases.append(m.astype(np.uint8))
    for seed in range(6):   # leaf-sized: one leaf of a 1080p scene, all leaves together, two disjoint leaves
        labels, _, _ = O.synthetic_scene(1080, 1920, 60 + seed)
        ids = [i for i in np.unique(labels) if i]
        cases.append((labels == ids[seed % len(ids)]).astype(np.uint8))
        cases.append((labels > 0).astype(np.uint8))
        cases.append(np.isin(labels, ids[:2]).astype(np.uint8))
    yy, xx = np.mgrid[0:600, 0:800]
    r, t = np.hypot(xx - 400, yy - 300), np.arctan2(yy - 300, xx - 400)
    cases.append((np.abs(((r / 12 - t / (2 * np.pi)) % 1.0) - 0.5) < 0.2).astype(np.uint8))          # spiral: one long border
    cases.append(((xx // 3 + yy // 3) % 2 == 0).astype(np.uint8))                                     # 3x3 checkerboard: corner-connected
    cases.append(((xx % 4 == 0) & (yy % 4 == 0)).astype(np.uint8))                                    # 30000 single pixels
    one = np.zeros((50, 70), np.uint8); one[20, 30] = 1
    cases.append(one)
    line = np.zeros((50, 70), np.uint8); line[25, 5:60] = 1
    cases.append(line)
    col = np.zeros((50, 70), np.uint8); col[5:45, 69] = 1
    cases.append(col)
    diag = np.zeros((64, 64), np.uint8); diag[np.arange(64), np.arange(64)] = 1
    cases.append(diag)
    return cases


@pytest.mark.parametrize("cap", [None, "64"])
def test_orientation_device_equals_host(L, cap, monkeypatch):
    """estimate_leaf_orientation (grasp_point_selector.py:718-752) on the device (lg_orient_kernel: runs, union-find, border
    following, hull chains, min-area rectangle) against the host analysis it replaces (lg_contour.cpp, LG_HOST_ORIENT=1; that
    one is held against the oracle bit for bit in tests/test_host_contour.py): the same five numbers as float32, for every
    case.  cap = 64 runs of scratch: most cases exceed it and must come back through the host hand-off."""
    monkeypatch.setenv("LG_HOST_ORIENT", "1")
    host = L.GraspPointSelector("cuda:0", load_model=False)
    monkeypatch.delenv("LG_HOST_ORIENT")
    if cap:
        monkeypatch.setenv("LG_ORIENT_CAP", cap)   # (read at lg_create: the handle keeps this cap for life)
    dev = L.GraspPointSelector("cuda:0", load_model=False)
    n_found = 0
    for k, m in enumerate(_orientation_cases()):
        want = host.estimate_leaf_orientation(m)
        got = dev.estimate_leaf_orientation(m)
        assert (want[0] is None) == (got[0] is None), k
        if want[0] is None:
            continue
        n_found += 1
        # float32 of the same float64 results; atan2 / fmod of the device library may differ from glibc in the last bit
        # of the double, i.e. never after rounding to float32 except on a rounding boundary
        assert got[0] == pytest.approx(want[0], abs=2e-7), (k, got, want)
        assert got[1:] == want[1:], (k, got, want)
    assert n_found > 130
    if cap is None:
        # an image taller than the device analysis takes (16384 rows): the scratch is dropped, the host analysis answers; and
        # back to an ordinary size afterwards
        tall = np.zeros((16400, 64), np.uint8)
        tall[100:16300, 10:30] = 1
        tall[5000:5010, 30:50] = 1
        assert dev.estimate_leaf_orientation(tall) == host.estimate_leaf_orientation(tall)
        small = _orientation_cases()[2]
        assert dev.estimate_leaf_orientation(small) == host.estimate_leaf_orientation(small)


def test_orientation_in_the_batched_path(L, monkeypatch):
    """lg_select_grasp with the orientation kernel beside the sweeps: theta and the score planes (the approach plane takes
    sin / cos of theta) equal the host-orientation path for a batch that mixes ordinary leaves, an empty mask, several
    components and a frame that overflows a small scratch (LG_ORIENT_CAP) and is handed back to the host threads."""
    H, W = 540, 720
    frames = [O.synthetic_scene(H, W, 70 + i) for i in range(6)]
    masks = np.stack([(f[0] == 1) for f in frames]).astype(np.uint8)
    masks[1][:] = 0
    masks[2] = (frames[2][0] > 0)
    rng = np.random.default_rng(3)
    masks[3] |= (rng.random((H, W)) > 0.98).astype(np.uint8)      # thousands of runs
    depths = np.stack([f[1] for f in frames])
    P = frames[0][2]
    monkeypatch.setenv("LG_HOST_ORIENT", "1")
    host = L.GraspPointSelector("cuda:0", load_model=False)
    monkeypatch.delenv("LG_HOST_ORIENT")
    monkeypatch.setenv("LG_ORIENT_CAP", "2048")   # (read at lg_create)
    dev = L.GraspPointSelector("cuda:0", load_model=False)
    out = []
    for sel in (host, dev):
        sel.set_camera_params(P)
        res, maps, valid = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(depths).cuda(),
                                                         return_maps=True)
        out.append((res, {k: v.cpu().numpy() for k, v in maps.items()}, valid.cpu().numpy(),
                    [r.theta for r in sel.last_results]))
    (res_h, maps_h, valid_h, th_h), (res_d, maps_d, valid_d, th_d) = out
    assert math.isnan(th_h[1]) and math.isnan(th_d[1])
    for b in (0, 2, 3, 4, 5):
        assert th_d[b] == pytest.approx(th_h[b], abs=2e-7), b
    assert res_d == res_h
    np.testing.assert_array_equal(valid_d, valid_h)
    for k in maps_h:
        np.testing.assert_allclose(maps_d[k], maps_h[k], rtol=0, atol=1e-6, err_msg=k)


def test_node_harness_end_to_end(L):
    """BASELINE config 1 analogue on the GPU path: wire arrays in, /optimal_leaf_grasp CSV out, equal to the
    oracle run through the same call sequence (leaf_grasp_node_v3.py:102-178)."""
    H, W = 720, 1280
    labels, depth, P = O.synthetic_scene(H, W, 5)
    hz = L.LeafGraspHarness(H, W, "cuda:0", load_model=False)
    hz.camera_info_callback(P.reshape(-1))
    csv = hz.process(labels.astype(np.uint16).reshape(-1), depth.reshape(-1))
    assert hz.leaf_grasp_done and csv is not None
    rl = O.RefOptimalLeafSelector()
    rl.set_camera_params(P)
    lid = rl.select_optimal_leaf(labels, depth)
    assert hz.last_leaf_id == lid
    rg = O.RefGraspPointSelector()
    rg.set_camera_params(P)
    p2, p3, pre = rg.select_grasp_point((labels == lid).astype(np.uint8), depth)
    vals = [float(v) for v in csv.split(",")]
    assert (int(vals[0]), int(vals[1])) == p2
    np.testing.assert_allclose(vals[2:5], p3, rtol=1e-5)
    np.testing.assert_allclose(vals[5:8], pre, rtol=1e-5)


def test_hybrid_grasp_selector_facade(L):
    H, W = 720, 1280
    labels, depth, P = O.synthetic_scene(H, W, 2)

    class FakeVLA:  # stands in for LLaVA (weights unavailable offline): prefers the LAST candidate
        def evaluate_candidates(self, image, candidates, instruction):
            return [i / max(1, len(candidates) - 1) for i in range(len(candidates))]

    hg = L.HybridGraspSelector("cuda:0", vla_scorer=FakeVLA(), load_model=False)
    hg.set_camera_params(P)
    cands = hg.generate_candidates(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())
    assert cands and all(c["mask"].dtype == torch.bool for c in cands)
    geo = [c["geometric_score"] for c in cands]
    assert geo == sorted(geo, reverse=True)
    img = np.zeros((H, W, 3), np.uint8)
    res = hg.select_grasp_point(img, cands, torch.from_numpy(depth).cuda())
    win = hg.last_selection
    # same decision as the reference's host classes fed the same numbers
    vla = FakeVLA().evaluate_candidates(img, cands, "")
    conf = L.ConfidenceManager().calculate_confidence(vla, geo)
    exp_win = L.HybridSelector("cpu").select_best_candidate(cands, geo, vla, conf)
    assert win["leaf_id"] == exp_win["leaf_id"]
    rg = O.RefGraspPointSelector()
    rg.set_camera_params(P)
    exp = rg.select_grasp_point((labels == win["leaf_id"]).astype(np.uint8), depth)
    assert res[0] == exp[0]
    np.testing.assert_allclose(res[1], exp[1], rtol=1e-5)
    # no VLA -> geometric arg-max (leaf_grasp_node_vla.py:138-139)
    hg2 = L.HybridGraspSelector("cuda:0", vla_scorer=None, load_model=False)
    hg2.set_camera_params(P)
    hg2.select_grasp_point(None, cands, torch.from_numpy(depth).cuda())
    assert hg2.last_selection["leaf_id"] == cands[0]["leaf_id"]
    assert hg2.select_grasp_point(None, [], None) == (None, None, None)


def test_hybrid_grasp_selector_with_the_llava_scorer_on_a_scripted_model(L):
    """BASELINE config 5's composition (leaf_grasp_node_vla.py:97-139,184-190) end to end on the HIP path with the real
    LLaVAScorer class driving a scripted (processor, model) pair -- the weights do not exist on this filesystem: candidates
    -> prompts -> generate / decode / parse -> normalise -> ConfidenceManager -> HybridSelector -> select_grasp_point on
    the winner's mask, against the same composition of the reference-pinned host classes and the oracle."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from leafgrasp_amd.vla_scorer import LLaVAScorer
    from scripted_llava import ScriptedModel, ScriptedProcessor
    H, W = 720, 1280
    labels, depth, P = O.synthetic_scene(H, W, 2)
    scorer = LLaVAScorer(device="cuda:0", model_path=None)
    hg = L.HybridGraspSelector("cuda:0", vla_scorer=scorer, load_model=False)
    hg.set_camera_params(P)
    dt = torch.from_numpy(depth).cuda()
    cands = hg.generate_candidates(torch.from_numpy(labels).cuda(), dt)
    assert len(cands) >= 3
    geo = [c["geometric_score"] for c in cands]
    img = np.zeros((H, W, 3), np.uint8)
    rg = O.RefGraspPointSelector()
    rg.set_camera_params(P)
    # scripts: the model prefers the geometrically WORST candidate strongly / answers garbage / fails on one candidate
    n = len(cands)
    scripts = [["assistant\n%.2f" % (0.05 + 0.9 * i / (n - 1)) for i in range(n)],
               ["assistant I cannot rate this"] * n,
               ["assistant 0.9", "!raise"] + ["assistant 0.2"] * (n - 2)]
    winners = []
    for script in scripts:
        scorer.processor, scorer.model = ScriptedProcessor(script), ScriptedModel(script)
        hg.confidence_manager = L.ConfidenceManager()
        res = hg.select_grasp_point(img, cands, dt)
        assert len(scorer.processor.prompts) == n and "Geometric score: %.3f" % geo[0] in scorer.processor.prompts[0]
        raw = []
        for t in script:   # llava_processor.py:92-101 applied by hand
            try:
                raw.append(0.5 if t == "!raise" else float(np.clip(float(t.split("assistant")[-1].strip()), 0.0, 1.0)))
            except ValueError:
                raw.append(0.5)
        raw = np.array(raw)
        vla = [0.5] * n if raw.std() < 1e-6 else ((raw - raw.min()) / (raw.max() - raw.min())).tolist()
        conf = L.ConfidenceManager().calculate_confidence(vla, geo)
        exp_win = L.HybridSelector("cpu").select_best_candidate(cands, geo, vla, conf)
        assert hg.last_selection["leaf_id"] == exp_win["leaf_id"]
        assert hg.last_selection["hybrid_score"] == pytest.approx(exp_win["hybrid_score"], rel=1e-12)
        winners.append(exp_win["leaf_id"])
        exp = rg.select_grasp_point((labels == exp_win["leaf_id"]).astype(np.uint8), depth)
        assert res[0] == exp[0]
        np.testing.assert_allclose(res[1], exp[1], rtol=1e-5)
        np.testing.assert_allclose(res[2], exp[2], rtol=1e-5)
    assert winners[0] != cands[0]["leaf_id"], "a confident scorer must be able to overrule the geometric arg-max"
    assert winners[1] == cands[0]["leaf_id"]          # constant 0.5 scores -> the geometric ranking decides


def test_hybrid_grasp_selector_with_stock_llava_classes_in_bf16_on_the_gpu(L, tmp_path):
    """BASELINE config 5 with everything real except the weights' values: the stock transformers LlavaNext classes, loaded from a
    local tiny random checkpoint (tests/tiny_llava.py) in bf16 on the MI355X, score the candidates inside HybridGraspSelector;
    the decision equals the same composition spelled out, the grasp point equals the oracle's for the winning leaf."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from leafgrasp_amd.vla_scorer import LLaVAScorer
    from test_host_logic import _tiny_llava_expected
    from tiny_llava import build_tiny_llava
    path = build_tiny_llava(str(tmp_path / "tiny_llava"))
    scorer = LLaVAScorer(device="cuda:0", model_path=path)               # bf16 by default, as config 5 names it
    assert scorer.model is not None and next(scorer.model.parameters()).dtype == torch.bfloat16
    assert next(scorer.model.parameters()).is_cuda
    H, W = 720, 1280
    labels, depth, P = O.synthetic_scene(H, W, 2)
    hg = L.HybridGraspSelector("cuda:0", vla_scorer=scorer, load_model=False)
    hg.set_camera_params(P)
    dt = torch.from_numpy(depth).cuda()
    cands = hg.generate_candidates(torch.from_numpy(labels).cuda(), dt)
    img = np.random.default_rng(1).integers(0, 255, (60, 80, 3), dtype=np.uint8)
    res = hg.select_grasp_point(img, cands, dt)
    vla, _ = _tiny_llava_expected(scorer, img, cands, "Select the best leaf for grasping")
    geo = [c["geometric_score"] for c in cands]
    conf = L.ConfidenceManager().calculate_confidence(vla, geo)
    exp_win = L.HybridSelector("cpu").select_best_candidate(cands, geo, vla, conf)
    assert hg.last_selection["leaf_id"] == exp_win["leaf_id"]
    rg = O.RefGraspPointSelector()
    rg.set_camera_params(P)
    exp = rg.select_grasp_point((labels == exp_win["leaf_id"]).astype(np.uint8), depth)
    assert res[0] == exp[0]
    np.testing.assert_allclose(res[1], exp[1], rtol=1e-5)


def test_leaf_workspace_survives_a_change_of_aspect(L):
    """the leaf stage's bit rows are H x ceil(W / 64) words -- 480 x 640 needs 4800 per frame, 640 x 480 needs
    5120 at the same pixel count.  One handle, both shapes, either order: statistics and selection equal the oracle."""
    sel = L.OptimalLeafSelector(torch.device("cuda:0"))
    n_sel = 0
    for shape in ((480, 640), (640, 480), (720, 960), (960, 720), (600, 450), (480, 640), (300, 1000), (1000, 300), (960, 720)):
        labels, depth, P = O.synthetic_scene(*shape, 7)
        sel.set_camera_params(P)
        ref = O.RefOptimalLeafSelector(field="edt")
        ref.set_camera_params(P)
        exp = ref.select_optimal_leaf(labels, depth)
        assert sel.select_optimal_leaf(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda()) == exp, shape
        if exp is not None:   # (a frame without a 10000-px leaf leaves _tall_leaves at its previous value, leaf_scorer.py:144-146,174)
            assert sel.get_tall_leaves() == ref.get_tall_leaves()
            n_sel += 1
        rows, _, _ = sel.leaf_statistics(torch.from_numpy(labels).cuda(), torch.from_numpy(depth).cuda())
        assert [r["id"] for r in rows] == np.unique(labels)[1:].tolist()
        for r in rows:
            lm = labels == r["id"]
            assert r["area"] == int(lm.sum()) and r["median_depth"] == np.median(depth[lm])
    assert n_sel >= 3


def test_leaf_selection_batch_equals_per_frame(L):
    """lg_leaf_stats_batch / select_optimal_leaves_batch / LeafGraspHarness.process_batch: B frames per call give exactly
    the per-frame results (statistics, extrema, chosen leaf, tall leaves, CSV)."""
    H, W = 540, 720                                      # large enough for leaves above the 10000 px area threshold
    frames = [O.synthetic_scene(H, W, 40 + i) for i in range(7)]
    P = frames[0][2]
    labels = np.stack([f[0] for f in frames]).astype(np.int16)
    labels[5][:] = 0                                     # a frame without leaves
    depths = np.stack([f[1] for f in frames])
    ols = L.OptimalLeafSelector("cuda:0")
    ols.set_camera_params(P)
    lab_d, dep_d = torch.from_numpy(labels).cuda(), torch.from_numpy(depths).cuda()
    batch = ols.leaf_statistics_batch(lab_d, dep_d)
    for b in range(len(frames)):
        single = ols.leaf_statistics(lab_d[b], dep_d[b])
        assert batch[b][1] == single[1] and batch[b][2] == single[2]
        assert len(batch[b][0]) == len(single[0])
        for x, y in zip(batch[b][0], single[0]):
            assert x["id"] == y["id"] and x["area"] == y["area"] and x["touches_border"] == y["touches_border"]
            assert x["sum_x"] == y["sum_x"] and x["sum_y"] == y["sum_y"] and x["median_depth"] == y["median_depth"]
            # f64 atomics: the accumulation order differs with the grid -> last-bit differences
            assert abs(x["sum_depth"] - y["sum_depth"]) <= 1e-9 * abs(y["sum_depth"]) + 1e-12
            assert abs(x["sum_ray"] - y["sum_ray"]) <= 1e-9 * abs(y["sum_ray"]) + 1e-12
    ids = ols.select_optimal_leaves_batch(lab_d, dep_d)
    want = [ols.select_optimal_leaf(lab_d[b], dep_d[b]) for b in range(len(frames))]
    assert ids == want and ids[5] is None and any(i is not None for i in ids)
    ref = O.RefOptimalLeafSelector()
    ref.set_camera_params(P)
    assert ids == [ref.select_optimal_leaf(labels[b], depths[b]) for b in range(len(frames))]
    hz = L.LeafGraspHarness(H, W, "cuda:0", load_model=False)
    hz.camera_info_callback(P.reshape(-1))
    hz.grasp_selector.set_cnn_state_dict(O.cnn_closed_form_params(0))
    csv_b = hz.process_batch(labels.astype(np.uint16).reshape(len(frames), -1), depths.reshape(len(frames), -1))
    csv_s = [hz.process(labels[b].astype(np.uint16).reshape(-1), depths[b].reshape(-1)) for b in range(len(frames))]
    assert csv_b == csv_s and csv_b[5] is None
    # the chunked path (leaf statistics of chunk k+1 in a worker thread beside selection + grasp pass of chunk k)
    for chunks in (1, 2, 3, len(frames)):
        assert hz.process_batch_device(lab_d, dep_d, chunks=chunks) == csv_s, chunks
        assert hz.last_leaf_ids == ids


def test_bench_two_ranks_one_device(tmp_path):
    """The multi-GPU launch of bench.py rehearsed on this one-GPU box: the driver's command line
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 ... bench.py --gpus 2 ...`) with both ranks on device 0 over
    gloo (LG_BENCH_ONE_DEVICE=1; the real run puts one rank per GPU over RCCL).  Frames are sharded, nothing is exchanged on the
    data path: rank 0 prints ONE JSON line whose value is the frames of BOTH ranks over the slowest rank's time."""
    import json
    import os
    import socket
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LG_BENCH_ONE_DEVICE="1")
    steps, batch = 3, 8
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", str(steps),
                          "--warmup", "1", "--batch", str(batch), "--height", "270", "--width", "360", "--full"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=repo)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == steps and res["scaling"] == "weak" and res["unit"] == "frames/s"
    assert res["config"]["frames_per_step_per_gpu"] == batch
    # whole-job value: 2 ranks x batch x steps frames over the (max over ranks) time
    assert res["value"] == pytest.approx(2 * batch * steps / (res["ms_per_step"] * steps * 1e-3), rel=2e-3)
    assert "cpu_baseline" not in res and "roofline" in res      # the CPU leg is rank 0 at N = 1 only


def test_bench_plain_run_dumps_its_results(L, tmp_path):
    """A plain bench.py run reports the headline only (no per-kernel figures or secondary legs), times exactly --steps steps,
    and --dump-outputs writes the last step's results: the triples select_grasp_points_batch returns for the same seeded
    frames on a fresh handle."""
    import json
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, H, W, steps = 8, 270, 360, 3
    out = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--batch", str(B), "--height", str(H), "--width", str(W), "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=repo)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["unit"] == "frames/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["value"] == pytest.approx(B * steps / (res["ms_per_step"] * steps * 1e-3), rel=2e-3)
    for key in ("kernels_ms", "roofline", "kernel_fracs", "mfma", "cpu_baseline", "configs", "node_sequence", "train_step"):
        assert key not in res, key

    import bench
    import synthetic_inputs as SI

    masks, depths, P, _ = bench.make_frames(B, H, W)
    sel = L.GraspPointSelector("cuda:0", load_model=False)
    sel.set_camera_params(P)
    sel.set_cnn_state_dict(SI.cnn_closed_form_params(seed=0))
    want = sel.select_grasp_points_batch(torch.from_numpy(masks).cuda(), torch.from_numpy(depths).cuda())
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("grasp_xy", "grasp_xyz", "pregrasp_xyz")}
    assert all(a.dtype == np.float64 and a.shape[0] == B for a in got.values())
    for b, (xy, xyz, pre) in enumerate(want):
        assert tuple(got["grasp_xy"][b]) == xy and tuple(got["grasp_xyz"][b]) == xyz
        assert np.isnan(got["pregrasp_xyz"][b]).all() if pre is None else tuple(got["pregrasp_xyz"][b]) == pre


@pytest.mark.parametrize("shape", [(360, 480), (270, 363)])
def test_grasp_points_for_leaves_equal_the_masks_path(L, shape):
    """lg_select_grasp_labels -- the node's `optimal_mask = mask_tensor == optimal_leaf_id` (leaf_grasp_node_v3.py:118) folded
    into the library's first pass over the frame -- against the comparison done by torch and select_grasp_points_batch on the
    bool masks: the same triples, frame by frame, for a width the 16-label vector pass takes and one it does not; a frame
    without a leaf id comes back as (None, None, None) (the node skips it), one whose id no pixel carries as the masks path's
    answer for an empty mask."""
    H, W = shape
    frames = [O.synthetic_scene(H, W, 90 + i) for i in range(5)]
    labels = torch.from_numpy(np.stack([f[0] for f in frames]).astype(np.int16)).cuda()
    depth = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    sel = L.GraspPointSelector("cuda:0", load_model=False)
    sel.set_camera_params(frames[0][2])
    sel.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))
    ids = [1, 2, None, 1, 31000]
    got = sel.select_grasp_points_for_leaves(labels, ids, depth)
    idt = torch.tensor([1, 2, -5, 1, 31000], dtype=torch.int16, device="cuda").reshape(-1, 1, 1)
    want = sel.select_grasp_points_batch(labels == idt, depth)
    assert got[2] == (None, None, None) and got[0][0] is not None
    assert [g for b, g in enumerate(got) if b != 2] == [w for b, w in enumerate(want) if b != 2]   # (an empty mask takes the reference's fall-through)
    # and again on the same handle with other ids (the id buffer and the mask workspace are reused)
    ids2 = [2, 1, 1, None, 3]
    idt2 = torch.tensor([2, 1, 1, -5, 3], dtype=torch.int16, device="cuda").reshape(-1, 1, 1)
    got2, want2 = sel.select_grasp_points_for_leaves(labels, ids2, depth), sel.select_grasp_points_batch(labels == idt2, depth)
    assert got2[3] == (None, None, None) and got2[:3] + got2[4:] == want2[:3] + want2[4:]
