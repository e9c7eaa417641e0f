"""detect_midrib and CLAHE on the device against the NumPy restatement (tests/midrib_ref.py): lg_clahe bit-exact, the
batched method's endpoints and status words with the library's own estimate_leaf_orientation values, batch == single calls,
and the mirror method's result types and never-raise convention."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import leafgrasp_amd as L  # noqa: E402

from tests import midrib_ref as R  # noqa: E402
from tests.midrib_scenes import scene_batch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def sel():
    return L.GraspPointSelector(DEV, load_model=False)


def _gray_frames(H, W, seed):
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, 256, (H, W), dtype=np.uint8)
    m, im = scene_batch(1, H, W, seed, kinds=("edge" if min(H, W) > 40 else "leaf",))
    return np.stack([rand, R.bgr2gray(im[0], m[0])])


@pytest.mark.parametrize("H,W", [(1080, 1920), (1080, 1440), (720, 1280), (1080, 1442), (517, 733), (5, 7)])
@pytest.mark.parametrize("clip", [0.0, 1.0, 3.0, 40.0])
@pytest.mark.parametrize("grid", [(8, 8), (4, 6)])
def test_clahe_bit_exact(H, W, clip, grid):
    g = _gray_frames(H, W, seed=H * 7 + W)
    got = L.clahe(torch.from_numpy(g).to(DEV), clip_limit=clip, tile_grid_size=grid).cpu().numpy()
    for b in range(g.shape[0]):
        exp = R.clahe(g[b], clip, grid)
        bad = np.argwhere(got[b] != exp)
        assert bad.size == 0, (b, len(bad), bad[:5].tolist())


def test_clahe_hand_worked_cases():
    tile = np.full((8, 8), 10, np.uint8)
    tile[5:] = 200
    out = L.clahe(torch.from_numpy(np.tile(tile, (2, 2))), 40.0, (2, 2)).cpu().numpy()
    assert (out == np.tile(np.where(tile == 10, 52, 243).astype(np.uint8), (2, 2))).all()
    img = np.array([[0, 0, 0, 1, 1, 2, 2, 2, 2, 3], [5] * 10], np.uint8)
    out = L.clahe(torch.from_numpy(img), 0.0, (1, 2)).cpu().numpy()
    assert out[0].tolist() == [76, 76, 76, 128, 128, 230, 230, 230, 230, 255]   # 76.5 rounds to 76


def test_clahe_unaligned_view_and_bad_arguments():
    g = _gray_frames(37, 53, seed=5)
    big = torch.zeros((2, 37, 54), dtype=torch.uint8, device=DEV)
    big[:, :, 1:] = torch.from_numpy(g).to(DEV)
    got = L.clahe(big[:, :, 1:], 3.0, (8, 8)).cpu().numpy()
    for b in range(2):
        assert (got[b] == R.clahe(g[b], 3.0, (8, 8))).all()
    with pytest.raises(L.LgError):
        L.clahe(torch.zeros((8, 8), dtype=torch.uint8, device=DEV), 3.0, (65, 8))
    with pytest.raises(L.LgError):
        L.clahe(torch.zeros((1, 8), dtype=torch.uint8, device=DEV), 3.0, (8, 8))


def _expected(sel, mask, img):
    return R.detect_midrib(mask, img, sel.estimate_leaf_orientation(mask))


@pytest.mark.parametrize("B,H,W", [(1, 1080, 1920), (7, 480, 640), (64, 240, 320)])
def test_detect_midrib_batch_matches_reference(sel, B, H, W):
    masks, imgs = scene_batch(B, H, W, seed=B * 1000 + H)
    got = sel.detect_midrib_batch(torch.from_numpy(masks).to(DEV), torch.from_numpy(imgs).to(DEV))
    assert len(got) == B
    statuses = set()
    for b in range(B):
        st, exp = _expected(sel, masks[b], imgs[b])
        statuses.add(st)
        assert sel.last_midrib_status[b] == st, (b, sel.last_midrib_status[b], st)
        assert got[b] == exp, (b, got[b], exp)
    if B >= 7:
        assert {0, 1, 2} <= statuses, statuses   # leaves, empty masks, leaves thinner than 6 px


def test_detect_midrib_batch_equals_single_calls(sel):
    masks, imgs = scene_batch(10, 200, 264, seed=77)
    batch = sel.detect_midrib_batch(masks, imgs)
    for b in range(10):
        assert sel.detect_midrib(masks[b], imgs[b]) == batch[b]
        assert sel.detect_midrib(torch.from_numpy(masks[b].astype(bool)), torch.from_numpy(imgs[b]).to(DEV)) == batch[b]


def test_detect_midrib_four_channels_ignore_alpha(sel):
    masks, imgs = scene_batch(5, 120, 160, seed=9)
    alpha = np.random.default_rng(0).integers(0, 256, imgs.shape[:3] + (1,), dtype=np.uint8)
    four = np.concatenate([imgs, alpha], axis=-1)
    assert sel.detect_midrib_batch(masks, four) == sel.detect_midrib_batch(masks, imgs)


def test_detect_midrib_mirror_types_and_errors(sel):
    masks, imgs = scene_batch(1, 300, 400, seed=3, kinds=("leaf",))
    r = sel.detect_midrib(masks[0], imgs[0])
    assert r is not None
    (x0, y0), (x1, y1) = r
    assert all(type(v) is int for v in (x0, y0, x1, y1))
    assert sel.detect_midrib(np.zeros((300, 400), np.uint8), imgs[0]) is None            # no contour
    assert sel.detect_midrib(masks[0], imgs[0][:, :200]) is None                           # shape mismatch
    assert sel.detect_midrib(masks[0], imgs[0][..., :2]) is None                           # C == 2
    assert sel.detect_midrib(masks[0], imgs[0].astype(np.float32)) is None                 # not uint8
    assert sel.detect_midrib(masks[0][0], imgs[0]) is None                                 # 1-D mask
    assert sel.detect_midrib(None, imgs[0]) is None
    assert sel.detect_midrib(masks[0], imgs[0]) == r                                       # the handle is still usable
