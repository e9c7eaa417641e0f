"""Deferred planes: a call that takes no plane and no validity back (sparse mode) does not store sdf, approach, isolation,
accessibility and stem; its plane kernel stores what top-k reads (and flatness, which cannot be recomputed bit for bit:
profiles/NOTES_deferred_planes.md) and the patch gather computes those five planes itself at the pixels of its windows.
Three assertions per case:

  patches          the patch of every scored slot (lg_debug_patch) equals, byte for byte, lg_gather_patches over the planes of
                   lg_score_maps for the same inputs and parameters at that call's candidate pixels -- for the candidates entry
                   (every candidate scored) and for the pruned pass of lg_select_grasp (survivors only);
  logits and rows  the logits (lg_debug_cnn_survivors) and the raw result rows equal those of a handle created under
                   LG_DEFER_PLANES=0 and those of the dense call (return_maps=True);
  stale state      a deferred call behind a dense call on the same handle, and the other way round.

The same under LG_NO_SKIP=2 / 3 and LG_SUBBATCH=2 (both handles created under the switch).  And: a fresh handle that has only
made sparse calls holds no workspace memory for the five planes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402

FIVE = ("sdf_score", "approach_score", "isolation_map", "accessibility_map", "stem_penalty")


@pytest.fixture(scope="module")
def L():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    return leafgrasp_amd


def _selector(L, P, monkeypatch=None, **env):
    """a fresh handle; the library reads its switches from the environment when the handle is created"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    for k in env:
        monkeypatch.delenv(k)
    sel.set_camera_params(P)
    sel.set_cnn_state_dict(O.cnn_closed_form_params(seed=0))
    return sel


def _largest_leaf(labels):
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    return int(ids[np.argmax(counts)])


def _frames(H, W, seeds):
    scenes = [O.synthetic_scene(H, W, s) for s in seeds]
    masks = np.stack([(lab == _largest_leaf(lab)) for lab, _, _ in scenes])
    depth = np.stack([d for _, d, _ in scenes])
    return masks, depth, scenes[0][2]


def _rows(sel, m, d, ip, return_maps=False, K=20):
    """raw result rows of one lg_select_grasp call, and the CNN pass behind it: {(frame, candidate): logit bytes} of the scored
    candidates and {(frame, candidate): patch slot}, over the call's sub-batches (one unless LG_SUBBATCH is set)"""
    sel.select_grasp_points_batch(m, d, return_maps=return_maps, image_processor=ip)
    torch.cuda.synchronize()
    s = sel.cnn_survivors()
    logits, slots = {}, {}
    for k in range(s["n_sub"]):
        base = k * s["sub_frames"] * K                # sub-batch k's entries of list and logits, and its patch slots, start here
        for j in range(int(s["counts"][k])):
            e = int(s["list"][base + j])
            bi = (k * s["sub_frames"] + e // K, e % K)
            logits[bi] = s["logits"][base + j].tobytes()
            slots[bi] = base + j
    return bytes(sel.last_results), logits, slots


def _check(L, monkeypatch, masks, depth, P, gaussian_size=5, env=None):
    """the three assertions; returns the candidate rows [B, K] and the survivors' (frame, candidate) pairs.  env: switches both
    handles are created under"""
    B, H, W = masks.shape
    K = 20
    ip = L.ImageProcessor(H, W, 21, gaussian_size)
    m, d = torch.from_numpy(masks).cuda(), torch.from_numpy(depth).cuda()
    env = env or {}
    sel = _selector(L, P, monkeypatch, **env)
    sel0 = _selector(L, P, monkeypatch, LG_DEFER_PLANES="0", **env)

    # ---- the reference: patches gathered from the planes of lg_score_maps, at the call's candidate pixels
    _, cands = sel.select_grasp_candidates_batch(m, d, image_processor=ip, top_k=K)
    torch.cuda.synchronize()
    xy = {}                                           # (frame, candidate) -> pixel
    for b in range(B):
        for r in cands[b]:
            if r["index"] >= 0:
                xy[(b, int(r["index"]))] = (int(r["x"]), int(r["y"]))
    got_all = {bi: sel.patch(bi[0] * K + bi[1]) for bi in xy}   # the candidates entry scores every candidate in its own slot
    maps, _, _ = sel0.score_maps(m, d, ip)
    want = {}
    for b in range(B):
        pts = sorted(bi for bi in xy if bi[0] == b)
        if pts:
            ref = sel0.gather_patches(m[b], d[b], {n: maps[n][b] for n in maps}, [xy[bi] for bi in pts]).cpu().numpy()
            for i, bi in enumerate(pts):
                want[bi] = ref[i]
    for bi in sorted(xy):
        assert got_all[bi].tobytes() == want[bi].tobytes(), ("candidates entry", bi, xy[bi], _first_diff(got_all[bi], want[bi]))

    # ---- the pruned pass of lg_select_grasp: survivors' patches, logits, rows
    rows, cnn, slots = _rows(sel, m, d, ip)
    pairs = sorted(slots)
    for bi in pairs:
        got = sel.patch(slots[bi])
        assert got.tobytes() == want[bi].tobytes(), ("survivor", slots[bi], bi, xy[bi], _first_diff(got, want[bi]))
    rows0, cnn0, _ = _rows(sel0, m, d, ip)
    assert cnn == cnn0 and rows == rows0, "LG_DEFER_PLANES=0"
    for name in FIVE:
        assert sel.ws_plane_bytes()[name] == 0 and sel0.ws_plane_bytes()[name] > 0, name
    # ---- stale state: dense behind deferred, deferred behind dense, on one handle
    rows_d, cnn_d, _ = _rows(sel, m, d, ip, return_maps=True)
    assert cnn == cnn_d and rows == rows_d, "dense call"
    rows_2, cnn_2, _ = _rows(sel, m, d, ip)
    assert cnn == cnn_2 and rows == rows_2, "deferred call behind the dense call"
    return cands, pairs, sel


def _first_diff(a, b):
    """(channel, row, column, got, want) of the first differing float and the differing floats per channel, for the message"""
    ia, ib = a.view(np.uint32), b.view(np.uint32)
    idx = np.argwhere(ia != ib)
    if idx.size == 0:
        return None
    c, y, x = idx[0]
    return int(c), int(y), int(x), float(a[c, y, x]), float(b[c, y, x]), (ia != ib).sum(axis=(1, 2)).tolist()


def test_leaves_across_constant_and_stencil_tiles(L, monkeypatch):
    """360 x 640, four frames: windows lie across state-0 and state-1 tiles and across rows of a stencil tile without a leaf pixel"""
    masks, depth, P = _frames(360, 640, [7, 8, 9, 10])
    cands, pairs, _ = _check(L, monkeypatch, masks, depth, P)
    assert len(pairs) > 0 and (cands["index"] >= 0).sum() > 40


def test_odd_width(L, monkeypatch):
    """301 x 517: W % 4 != 0, the instantiation without 16-byte accesses; partial last tile row and column"""
    masks, depth, P = _frames(301, 517, [40, 41, 42, 43])
    _check(L, monkeypatch, masks, depth, P)


def test_corner_leaves_empty_mask_and_a_frame_without_orientation(L, monkeypatch):
    """leaves in the top-left and bottom-right corners (reflect padding of the stencil meets replicate padding of the window), an
    empty mask (no orientation: has_angle = 0), and a one-pixel mask in the corner the fall-through picks start from"""
    H, W = 360, 640
    masks, depth, P = _frames(H, W, [7, 8, 9, 10])
    masks[:] = False
    masks[1, :45, :45] = True                            # every pixel of it is picked or suppressed by a pick within 10 px
    masks[2, H - 70:, W - 133:] = True
    masks[3, H - 2, W - 2] = True
    cands, _, sel = _check(L, monkeypatch, masks, depth, P)
    assert np.isnan(sel.last_results[0].theta)
    assert not np.isnan(sel.last_results[1].theta)
    for b, (cx, cy) in ((1, (0, 0)), (3, (W - 1, H - 1))):   # scored windows that reach over the corner
        ok = cands[b]["index"] >= 0
        assert (np.maximum(np.abs(cands[b]["x"][ok] - cx), np.abs(cands[b]["y"][ok] - cy)) < 16).any(), b


def test_uint8_mask_with_candidates_at_every_border(L, monkeypatch):
    """a uint8 mask (its border candidates are scored): one leaf against each border, candidates closer than 16 px to it"""
    H, W = 200, 328
    _, depth, P = _frames(H, W, [50, 51, 52, 53])
    masks = np.zeros((4, H, W), np.uint8)
    masks[0, :60, 120:200] = 1
    masks[1, H - 60:, 120:200] = 1
    masks[2, 70:150, :60] = 1
    masks[3, 70:150, W - 60:] = 1
    cands, _, _ = _check(L, monkeypatch, masks, depth, P)
    near = [cands[0]["y"] < 16, cands[1]["y"] >= H - 16, cands[2]["x"] < 16, cands[3]["x"] >= W - 16]
    for b in range(4):
        assert (near[b] & (cands[b]["index"] >= 0) & (cands[b]["scored"] != 0)).any(), b


@pytest.mark.parametrize("gaussian_size", [1, 3, 5, 7])
def test_every_stencil_radius(L, monkeypatch, gaussian_size):
    masks, depth, P = _frames(200, 328, [50, 51])
    masks[1] = False
    masks[1, :80, :100] = True        # and a corner leaf at every radius
    _check(L, monkeypatch, masks, depth, P, gaussian_size)


def test_small_squares_with_picks_on_constant_tiles(L, monkeypatch):
    H, W = 256, 384
    masks, depth, P = _frames(H, W, [11, 12, 13])
    for b, (y, x, r) in enumerate([(100, 200, 3), (30, 40, 7), (200, 350, 9)]):
        masks[b] = False
        masks[b, y - r:y + r + 1, x - r:x + r + 1] = True
    _check(L, monkeypatch, masks, depth, P)


@pytest.mark.parametrize("env", [{"LG_NO_SKIP": "2"}, {"LG_NO_SKIP": "3"}, {"LG_SUBBATCH": "2"}],
                         ids=["no_wave_shortcut", "no_skip_at_all", "subbatch_2"])
def test_switches_keep_working(L, monkeypatch, env):
    """LG_NO_SKIP bit 2: the gather's predicate is always true, like the plane kernel's (every zero is (...) * 0); bit 1: every
    tile has state 1.  LG_SUBBATCH=2 on five frames: three sub-batches, the gather of a later one takes its own plane-launch
    arguments and its patch slots start behind the earlier ones'."""
    masks, depth, P = _frames(200, 328, [60, 61, 62, 63, 64])
    _check(L, monkeypatch, masks, depth, P, env=env)


def test_a_handle_of_sparse_calls_holds_no_deferred_planes(L):
    masks, depth, P = _frames(200, 328, [50, 51])
    m, d = torch.from_numpy(masks).cuda(), torch.from_numpy(depth).cuda()
    sel = _selector(L, P)
    sel.select_grasp_points_batch(m, d)
    sel.select_grasp_candidates_batch(m, d)
    torch.cuda.synchronize()
    held = sel.ws_plane_bytes()
    assert all(held[n] == 0 for n in FIVE), held
    assert held["distance_map"] == held["traditional_score"] == held["flatness_map"] == 2 * 200 * 328 * 4, held
