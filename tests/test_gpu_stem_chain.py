"""The stem words by two chains of nested spans on the device (lg_stem_chain_kernel; the identity and the per-word code:
tests/test_stem_chain_math.py): lg_score_maps' stem and validity planes equal the oracle's bit for bit, as in
tests/test_gpu_stem_window.py, for stem_se in {1, 2, 3, 29, 30, 31, 63, 64} at 35 x 130, 48 x 200, 96 x 320 and 20 x 1100 (a
bounding box more than eight words wide), for leaves above, across and inside the bottom region and on both borders, for a
batch of nine frames with an empty mask and a full one, and on one handle for a small leaf after a large one and a leaf above
the bottom region after one inside it (every word of the plane is written on every call).  For each mask the triple of
select_grasp_points_batch (sparse planes) equals the triple of the same call with return_maps=True (every plane).  Every test
runs on a handle of the default form and on one created under LG_STEM_ALGO=0 (the per-row kernel): both give the oracle's
planes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import param_oracle as PO  # noqa: E402
from tests import param_sets as PS  # noqa: E402

SIZES = [(35, 130), (48, 200), (96, 320), (20, 1100)]
STEM_SE = [1, 2, 3, 29, 30, 31, 63, 64]
EDGE = 2.0   # min_edge_distance: small enough for these leaves to keep valid pixels
# one handle takes them in this order: a small leaf after a large one, a leaf above the bottom region after one inside it
ORDER = ["large", "small", "in the bottom rows", "above the bottom region", "across its first row", "left and right borders",
         "small"]


def _leaves(H, W, bs):
    """name -> mask; bs = first row of the bottom region"""
    yy, xx = np.mgrid[0:H, 0:W]
    rough = ((xx % 23 != 5) | (yy % 17 != 4)).astype(np.uint8)   # a few zero pixels inside the leaves

    def leaf(y0, y1, x0, x1):   # inclusive
        m = np.zeros((H, W), np.uint8)
        m[max(0, y0):min(H - 1, y1) + 1, x0:x1 + 1] = 1
        return m & rough
    return {
        "above the bottom region": leaf(1, bs - 2, W // 5, W - W // 3),
        "across its first row": leaf(bs - 25, bs + 4, 70, W - 9),
        "in the bottom rows": leaf(max(bs, H - 7), H - 1, 3, W // 2 + 40),
        "left and right borders": leaf(bs - 20, H - 2, 0, W - 1),
        "large": leaf(2, H - 1, 1, W - 2),
        "small": leaf(bs - 3, bs + 5, W - 40, W - 30),
    }


def _params(**changes):
    return PS.params_of({"min_edge_distance": EDGE, **changes})


@pytest.fixture(scope="module", params=[None, "0"], ids=["chains", "LG_STEM_ALGO=0"])
def algo(request):
    return request.param


def _selector(P, algo):
    import leafgrasp_amd as L

    assert torch.cuda.is_available()
    old = os.environ.get("LG_STEM_ALGO")
    try:   # the option is read when a handle is created
        os.environ.pop("LG_STEM_ALGO", None)
        if algo is not None:
            os.environ["LG_STEM_ALGO"] = algo
        sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    finally:
        os.environ.pop("LG_STEM_ALGO", None)
        if old is not None:
            os.environ["LG_STEM_ALGO"] = old
    sel.set_camera_params(P)
    for k, v in _params().items():
        if k not in ("min_edge_distance", "gaussian_size", "mask_is_bool"):
            setattr(sel.params, k, v)
    sel.min_edge_distance = EDGE
    return sel


_REFS = {}


def _scene(size):
    """(depth, camera, name -> (mask, {stem_se: (stem, valid)})), computed once for both arms"""
    if size not in _REFS:
        H, W = size
        _, depth, P = O.synthetic_scene(H, W, seed=4)
        masks = _leaves(H, W, H - H // 3)
        masks["empty"] = np.zeros((H, W), np.uint8)
        masks["full"] = np.ones((H, W), np.uint8)
        per = {}
        for name, m in masks.items():
            base = PO.oracle(P, _params())
            dist = O.distance_transform(m, 5, init_dist0=base.init_dist0)   # (the validity plane's other input: not stem_se's)
            by_se = {}
            for k in STEM_SE:
                ref = PO.oracle(P, _params(stem_se=k))
                stem = ref._calculate_stem_penalty(m)
                by_se[k] = (stem, ref._get_valid_regions(m, {"distance_map": dist, "stem_penalty": stem}))
            per[name] = (m, by_se)
        _REFS[size] = (depth, P, per)
    return _REFS[size]


def _check_planes(sel, masks, depth, want, what):
    """masks [B, H, W]; want = [(stem, valid)] per frame"""
    B = masks.shape[0]
    maps, v, _ = sel.score_maps(torch.from_numpy(masks).cuda(), torch.from_numpy(np.stack([depth] * B)).cuda())
    got, v = maps["stem_penalty"].cpu().numpy(), v.cpu().numpy().astype(bool)
    for b in range(B):
        print(f"{what} [{b}]: stem {int(got[b].sum())} / {int(want[b][0].sum())} px, valid {int(v[b].sum())} / {int(want[b][1].sum())} px")
        np.testing.assert_array_equal(got[b], want[b][0], err_msg=f"{what} [{b}] stem")
        np.testing.assert_array_equal(v[b], want[b][1], err_msg=f"{what} [{b}] valid")


def _check_triples(sel, masks, depth, what):
    """sparse planes against every plane; returns the frames with a grasp point"""
    B = masks.shape[0]
    m, d = torch.from_numpy(masks).cuda(), torch.from_numpy(np.stack([depth] * B)).cuda()
    sparse = sel.select_grasp_points_batch(m, d)
    dense, _, _ = sel.select_grasp_points_batch(m, d, return_maps=True)
    np.testing.assert_equal(sparse, dense, err_msg=what)
    return sum(t[0] is not None for t in sparse)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_and_validity_planes_for_every_ellipse(size, algo):
    depth, P, per = _scene(size)
    H, W = size
    m_across = per["across its first row"][0]
    xs = np.nonzero(m_across.any(axis=0))[0]
    if W > 1000:
        assert (xs[-1] >> 6) - (xs[0] >> 6) + 1 > 8          # a box more than eight words wide
    for k in STEM_SE:   # nothing here compares zeros with zeros only
        assert per["above the bottom region"][0].sum() > 0 and per["above the bottom region"][1][k][0].sum() == 0
        for n in ("across its first row", "in the bottom rows", "left and right borders", "large", "small"):
            assert per[n][1][k][0].sum() > 0, (n, k)
    assert per["across its first row"][1][3][0].sum() < m_across.sum()
    sel = _selector(P, algo)
    found = 0
    for k in STEM_SE:
        sel.params.stem_se = k
        for n in ORDER:
            m, by_se = per[n]
            _check_planes(sel, m[None], depth, [by_se[k]], f"{size} stem_se {k} {n}")
            found += _check_triples(sel, m[None], depth, f"{size} stem_se {k} {n}")
    assert found > 0


@pytest.mark.parametrize("k", [30, 63])
def test_batch_of_nine_with_an_empty_and_a_full_mask(k, algo):
    size = (48, 200)
    depth, P, per = _scene(size)
    names = ["large", "above the bottom region", "empty", "small", "in the bottom rows", "full", "left and right borders",
             "across its first row", "small"]
    masks = np.stack([per[n][0] for n in names])
    assert per["full"][1][k][0].sum() > 0 and per["empty"][1][k][0].sum() == 0
    sel = _selector(P, algo)
    sel.params.stem_se = k
    _check_planes(sel, masks, depth, [per[n][1][k] for n in names], f"batch stem_se {k}")
    assert _check_triples(sel, masks, depth, f"batch stem_se {k}") > 0
    # the same handle, one frame: the words of the other eight frames' planes are no longer looked at, those of frame 0 are new
    _check_planes(sel, masks[3:4], depth, [per["small"][1][k]], f"one frame after the batch, stem_se {k}")
