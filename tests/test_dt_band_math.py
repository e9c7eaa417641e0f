"""The two identities the band form of the sweep-free distance transform rests on (lg_dtseed_kernel's seed pairs +
lg_dtband_kernel, csrc/lg_dt.hip), checked on the CPU against the integers of the oracle's two-pass chamfer transform:
  1. with h = the run distance of a pixel's own row, U(y) = min(A h, the 5 x 5 stencil over U(y - 1), U(y - 2)) is the distance to
     the nearest zero pixel at or above the row -- no in-row scan; the mirrored D, and d = min(U, D);
  2. the same recurrence started from the TRUE d on two adjacent rows, downwards from the pair above a band and upwards from the
     pair below it, gives the true d on every row between -- also tile-locally, when seeds and h are cut off 2 columns per band
     row beyond the tile's edges.
NumPy emulation of the arithmetic only -- the kernels are compared with the oracle in tests/test_gpu_dt_bands.py."""
import numpy as np
import pytest

from oracle import lg_oracle as O
from tests.test_dt_search_math import _cases

A, B, C = 65536, 91750, 143976
CAP = 16383
INF = 0x3FFFFFFF   # "no path": rows / columns outside the image, and everything a tile does not see


def _ref(mask):
    return O.distance_transform(mask, 5, return_fix=True)[1].astype(np.int64)


def _runs(mask):
    """h of EVERY row (A * CAP in a row without a zero pixel: an upper bound that beats nothing)."""
    H, W = mask.shape
    h = np.full((H, W), CAP, np.int64)
    for y in range(H):
        z = np.nonzero(mask[y] == 0)[0]
        if z.size:
            h[y] = np.abs(np.arange(W)[:, None] - z[None, :]).min(1)
    return h


def _sh(a, k):   # a[x + k], "no path" beyond the ends
    out = np.full_like(a, INF)
    if k > 0:
        out[:-k] = a[k:]
    else:
        out[-k:] = a[:k]
    return out


def _step(p1, p2, ah):   # one row of the recurrence: p1 / p2 = the rows one / two steps back, ah = A * h of the row itself
    mc = np.minimum(np.minimum(_sh(p1, 2), _sh(p1, -2)), np.minimum(_sh(p2, 1), _sh(p2, -1))) + C
    mb = np.minimum(_sh(p1, 1), _sh(p1, -1)) + B
    return np.minimum(np.minimum(ah, p1 + A), np.minimum(mb, mc))


def _row(a, y, fill=INF):   # row y of a, `fill` outside the image
    return a[y] if 0 <= y < a.shape[0] else np.full(a.shape[1], fill, np.int64)


def _band(seed, ah, s, n):
    """Rows s .. s + n - 1 from the seed pairs (s - 2, s - 1) and (s + n, s + n + 1): min of the two runs."""
    up = []
    p2, p1 = _row(seed, s - 2), _row(seed, s - 1)
    for y in range(s, s + n):
        p2, p1 = p1, _step(p1, p2, _row(ah, y))
        up.append(p1)
    out = [None] * n
    p2, p1 = _row(seed, s + n + 1), _row(seed, s + n)
    for i in range(n - 1, -1, -1):
        p2, p1 = p1, _step(p1, p2, _row(ah, s + i))
        out[i] = np.minimum(up[i], p1)
    return out


def _big_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        H, W = int(rng.integers(40, 141)), int(rng.integers(130, 331))
        yy, xx = np.mgrid[:H, :W]
        kind = t % 4
        if kind == 0:
            th = rng.random() * np.pi
            u = (xx - W / 2) * np.cos(th) + (yy - H / 2) * np.sin(th)
            v = -(xx - W / 2) * np.sin(th) + (yy - H / 2) * np.cos(th)
            m = (u / (W / 2.2)) ** 2 + (v / (H / 3)) ** 2 < 1
        elif kind == 1:
            m = rng.random((H, W)) < 0.97
        elif kind == 2:
            m = np.ones((H, W), bool)
            m[rng.integers(0, H), rng.integers(0, W)] = False
        else:
            m = np.abs((yy - H / 2) - (xx - W / 2) * rng.uniform(-0.6, 0.6)) < rng.integers(3, 30)
            m[:, :3] = False
        out.append(m.astype(np.uint8))
    return out


def test_identity_1_stencil_over_run_distances_is_the_transform():
    cases = _cases(240, 5)
    assert len(cases) > 200
    bad = 0
    for mask in cases:
        H, W = mask.shape
        ref, ah = _ref(mask), A * _runs(mask)
        U, D = np.empty_like(ref), np.empty_like(ref)
        p1 = p2 = np.full(W, INF, np.int64)
        for y in range(H):
            p2, p1 = p1, _step(p1, p2, ah[y])
            U[y] = p1
        p1 = p2 = np.full(W, INF, np.int64)
        for y in range(H - 1, -1, -1):
            p2, p1 = p1, _step(p1, p2, ah[y])
            D[y] = p1
        bad += int((np.minimum(U, D) != ref).sum())
    assert bad == 0


@pytest.mark.parametrize("n", [3, 6, 14])
def test_identity_2_bands_between_exact_row_pairs(n):
    """Seed pairs every P = n + 2 rows; first pair at row 0, or above it (rows -2, -1: "no path"), or straddling it; the last band
    is cut by the image's last rows whenever (H - first) % P allows."""
    P = n + 2
    bad = checked = 0
    for t, mask in enumerate(_cases(90, 7)):
        H, W = mask.shape
        ref, ah = _ref(mask), A * _runs(mask)
        first = (0, -2, -1)[t % 3]
        for s in range(first + 2, H, P):
            for i, r in enumerate(_band(ref, ah, s, n)):
                if s + i < H:
                    bad += int((r != ref[s + i]).sum())
                    checked += 1
    assert checked and bad == 0


@pytest.mark.parametrize("n", [7, 14])
def test_identity_2_tile_local_with_two_columns_of_halo_per_band_row(n):
    P = n + 2
    bad = tiles = 0
    for t, mask in enumerate(_big_cases(48, 13)):
        H, W = mask.shape
        assert H <= 140 and W <= 330
        ref, ah = _ref(mask), A * _runs(mask)
        first = (0, -2)[t % 2]
        for x0 in range(0, W, 64):
            xa, xb = max(x0 - 2 * n, 0), min(x0 + 64 + 2 * n, W)   # what the tile sees; the image's own edge is a real edge
            for s in range(first + 2, H, P):
                got = _band(ref[:, xa:xb], ah[:, xa:xb], s, n)
                for i, r in enumerate(got):
                    if s + i < H:
                        bad += int((r[x0 - xa:x0 - xa + 64] != ref[s + i, x0:x0 + 64]).sum())
                tiles += 1
    assert tiles and bad == 0
