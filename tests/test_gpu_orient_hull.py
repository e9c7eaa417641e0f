"""Step E of the orientation kernel in two levels (every row against its block of 16 rows, then the blocks' vertices against
each other; the identity: tests/test_hull_two_level_math.py) against the host analysis it replaces (LG_HOST_ORIENT=1):
estimate_leaf_orientation must return the same five values, bit for bit.  The masks put component heights on the block edges
(15, 16, 17, 33 rows), past one row per thread (300 rows), and on profiles with many vertices (a disc), with many collinear
rows (rectangle, diamond), with long flat runs (staircase) and with specks beside the leaf; a handle with a small run scratch
(LG_ORIENT_CAP) checks that the kernel's LDS is sized for step E's lists and not for the scratch alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _masks():
    out = {}
    yy, xx = np.mgrid[0:360, 0:420]
    for h in (15, 16, 17, 33, 300):    # a slanted ellipse h rows tall
        cy, b = 20 + (h - 1) / 2.0, (h - 1) / 2.0 + 0.2
        out[f"{h} rows"] = ((((xx - 200 - 0.3 * (yy - cy)) / 90.0) ** 2 + ((yy - cy) / b) ** 2) <= 1.0)
    out["disc of radius 100"] = np.hypot(yy - 170, xx - 200) <= 100
    m = np.zeros(yy.shape, bool); m[40:300, 90:330] = True
    out["rectangle"] = m
    out["diamond"] = (np.abs(yy - 170) + np.abs(xx - 200)) <= 120
    out["flat diamond"] = (3 * np.abs(yy - 170) + np.abs(xx - 200)) <= 150
    out["staircase"] = (xx >= 40 + (yy // 9) * 7) & (xx <= 150 + (yy // 13) * 11) & (yy >= 12) & (yy < 340)
    rng = np.random.default_rng(8)
    leaf = ((((xx - 180) / 120.0) ** 2 + ((yy - 150 - 0.4 * (xx - 180)) / 50.0) ** 2) <= 1.0)
    out["leaf plus specks"] = leaf | (rng.random(yy.shape) > 0.997)
    out["ragged blob"] = leaf & ((xx + 2 * yy) % 17 != 0) | (np.hypot(yy - 150, xx - 180) < 30)
    return {k: v.astype(np.uint8) for k, v in out.items()}


@pytest.fixture(scope="module")
def handles():
    import os

    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    old = {k: os.environ.get(k) for k in ("LG_HOST_ORIENT", "LG_ORIENT_CAP")}
    try:   # the options are read when a handle is created (lg_create) and stay with it: lg_debug_options shows them
        os.environ.pop("LG_ORIENT_CAP", None)
        os.environ["LG_HOST_ORIENT"] = "1"
        host = L.GraspPointSelector("cuda:0", load_model=False)
        del os.environ["LG_HOST_ORIENT"]
        dev = L.GraspPointSelector("cuda:0", load_model=False)
        os.environ["LG_ORIENT_CAP"] = "320"   # parent[] takes 1280 bytes of LDS, step E's rows and lists of 300 rows 2480
        small = L.GraspPointSelector("cuda:0", load_model=False)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return host, dev, small


@pytest.fixture(scope="module")
def wanted(handles):
    """name -> (mask, the host analysis' answer), computed once"""
    return {k: (m, handles[0].estimate_leaf_orientation(m)) for k, m in _masks().items()}


@pytest.mark.parametrize("name", list(_masks()))
def test_five_values_equal_the_host_analysis(handles, wanted, name):
    from leafgrasp_amd._lib import lib

    m, want = wanted[name]
    assert lib.lg_orientation_note(handles[1]._h) == b""   # the device analysis is set up
    got = handles[1].estimate_leaf_orientation(m)
    print(name, got, want)
    assert want[0] is not None
    assert got == want


def test_each_handle_holds_the_options_it_was_created_under(handles):
    host, dev, small = (h.options() for h in handles)
    assert (host["LG_HOST_ORIENT"], dev["LG_HOST_ORIENT"], small["LG_HOST_ORIENT"]) == (1, 0, 0)
    assert (host["LG_ORIENT_CAP"], dev["LG_ORIENT_CAP"], small["LG_ORIENT_CAP"]) == (16384, 16384, 320)


def _runs(m):
    return int((np.diff(np.pad(m.astype(np.int8), ((0, 0), (1, 0))), axis=1) == 1).sum())


def test_the_small_cap_is_in_force(handles):
    """A 300 x 200 mask with more runs than the small scratch holds and fewer than the default one: select_grasp_point hands the
    frame back to the host analysis on `small` (lg_debug_orient_redo = 1) and not on `dev`; both return what the handle that
    analyses every frame on the host returns."""
    import ctypes as C

    from leafgrasp_amd._lib import lib
    from oracle import lg_oracle as O

    H, W = 300, 200
    labels, depth, P = O.synthetic_scene(H, W, 5)
    yy, xx = np.mgrid[0:H, 0:W]
    leaf = ((((xx - 100) / 70.0) ** 2 + ((yy - 140 - 0.4 * (xx - 100)) / 50.0) ** 2) <= 1.0)
    m = (leaf & ((xx + 2 * yy) % 17 != 0) | (np.hypot(yy - 140, xx - 100) < 30)).astype(np.uint8)   # the ragged blob at this size
    assert 320 < _runs(m) < 16384
    mt, dt = torch.from_numpy(m.astype(bool)).cuda(), torch.from_numpy(depth).cuda()
    res, redo = [], []
    for h in handles:
        h.set_camera_params(P)
        res.append(h.select_grasp_point(mt, dt, None))
        n = C.c_int32(-1)
        assert lib.lg_debug_orient_redo(h._h, C.byref(n)) == 0
        redo.append(n.value)
        assert lib.lg_orientation_note(h._h) == b""
    print(_runs(m), res, redo)
    assert res[0][0] is not None
    assert redo == [0, 0, 1]          # host: analyses every frame anyway; dev: the kernel; small: handed back
    assert res[1] == res[0] and res[2] == res[0]


def test_small_run_scratch_at_300_rows(handles, wanted):
    """one run per row: 300 runs fit the scratch of 320, so the kernel analyses the frame itself -- with step E's lists in LDS"""
    from leafgrasp_amd._lib import lib

    small = handles[2]
    assert lib.lg_orientation_note(small._h) == b""
    for name in ("300 rows", "rectangle", "diamond"):
        m, want = wanted[name]
        assert _runs(m) <= 320 and m.any(axis=1).sum() >= 240, name
        assert small.estimate_leaf_orientation(m) == want, name
    yy, xx = np.mgrid[0:300, 0:200]   # a frame of H = 300 that the leaf fills from the first row to the last
    m = ((((xx - 100 - 0.2 * (yy - 149.5)) / 60.0) ** 2 + ((yy - 149.5) / 149.7) ** 2) <= 1.0).astype(np.uint8)
    assert m.any(axis=1).all()
    want = handles[0].estimate_leaf_orientation(m)
    assert want[0] is not None
    assert small.estimate_leaf_orientation(m) == want
    assert handles[1].estimate_leaf_orientation(m) == want
