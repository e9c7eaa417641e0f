"""Max d_out along a frame border line by the pruned search (lg_border_line_max: the code lg_dout_border_kernel runs) against
the brute-force maximum: every candidate p in {lo .. lo + n - 1, 0, len - 1} against every profile entry, with the 5 x 5 chamfer
norm written out from its 16.16 integers.  The search stops a candidate once its running minimum cannot raise the maximum, or
once no farther entry can lower the minimum; both rules rest on the norm growing with either argument, which is tested too."""
import ctypes as C

import numpy as np
import pytest

A5, B5, C5 = 65536, 91750, 143976   # 1, 1.4, 2.1969 in 16.16 fixed point


def norm5(dx, dy):
    a, b = np.maximum(dx, dy).astype(np.int64), np.minimum(dx, dy).astype(np.int64)
    return np.where(2 * b <= a, (a - 2 * b) * A5 + b * C5, (a - b) * C5 + (2 * b - a) * B5)


def brute(prof, lo, length):
    prof = np.asarray(prof, np.int64)
    n = len(prof)
    pos = lo + np.arange(n)
    ok = prof >= 0
    if not ok.any():
        return 0xFFFFFFFF
    cand = np.concatenate([pos, [0, length - 1]])
    d = norm5(np.abs(cand[:, None] - pos[ok][None, :]), np.broadcast_to(prof[ok][None, :], (len(cand), int(ok.sum()))))
    return int(d.min(axis=1).max())


def search(prof, lo, length):
    from leafgrasp_amd import _lib

    p = np.ascontiguousarray(prof, np.int32)
    out = C.c_uint32(0)
    rc = _lib.lib.lg_border_line_max(p.ctypes.data_as(C.POINTER(C.c_int32)), len(p), lo, length, C.byref(out))
    assert rc == 0
    return out.value


def _profiles(n, rng):
    """name -> profile of n entries (distances from the border; -1: no leaf pixel in that line position)"""
    i = np.arange(n)
    out = {}
    out["random"] = rng.integers(0, 900, n)
    out["random small"] = rng.integers(0, 4, n)
    c, r = (n - 1) / 2.0, max(n / 2.0, 1.0)
    out["elliptical"] = np.round(300 + 180 * (1 - np.sqrt(np.clip(1 - ((i - c) / r) ** 2, 0, 1)))).astype(int)
    u = np.full(n, 5); u[n // 6:n - n // 6] = 700    # a U open towards the border: its inside is far from every entry nearby
    out["u open to the border"] = u
    u = np.full(n, 3); u[1:n - 1] = 1500
    out["deep u"] = u
    g = rng.integers(0, 600, n); g[rng.random(n) < 0.5] = -1; g[rng.integers(n)] = 17
    out["gaps"] = g
    g = np.full(n, -1); g[0] = 40; g[n - 1] = 2      # two components with empty positions between them
    out["two ends only"] = g
    s = np.full(n, -1); s[rng.integers(n)] = int(rng.integers(0, 500))
    out["single entry"] = s
    out["all equal"] = np.full(n, int(rng.integers(0, 800)))
    out["all zero"] = np.zeros(n, int)
    out["ramp"] = i * 2
    out["ramp down"] = (n - 1 - i) * 3
    return out


SIZES = [1, 2, 3, 255, 256, 257, 600]


@pytest.mark.parametrize("n", SIZES)
def test_pruned_search_equals_brute_force(n):
    rng = np.random.default_rng(1000 + n)
    checked = 0
    for name, prof in _profiles(n, rng).items():
        for lo, length in ((0, n), (0, n + 333), (419, n + 419), (37, n + 37 + 880)):   # lo = 0, lo + n = len, both, neither
            got, exp = search(prof, lo, length), brute(prof, lo, length)
            assert got == exp, (name, n, lo, length, got, exp)
            checked += 1
    for k in range(24):   # more random ones, of mixed density and depth
        prof = rng.integers(0, int(rng.integers(1, 1200)), n)
        prof[rng.random(n) < rng.uniform(0, 0.9)] = -1
        lo = int(rng.integers(0, 500))
        length = lo + n + int(rng.integers(0, 500))
        assert search(prof, lo, length) == brute(prof, lo, length), ("random", n, k)
        checked += 1
    assert checked == 12 * 4 + 24


def test_maximum_inside_the_span():
    """the U's maximum is attained by a span candidate, not by an end of the line: the span search decides the result"""
    n, lo, length = 600, 100, 800
    prof = np.full(n, 5); prof[100:500] = 700
    pos = lo + np.arange(n)
    ends = norm5(np.abs(np.array([0, length - 1])[:, None] - pos[None, :]), np.broadcast_to(prof[None, :], (2, n))).min(axis=1).max()
    exp = brute(prof, lo, length)
    assert exp > ends
    assert search(prof, lo, length) == exp


def test_no_entry_and_bad_arguments():
    from leafgrasp_amd import _lib

    assert search(np.full(7, -1), 3, 20) == 0xFFFFFFFF
    fn = _lib.lib.lg_border_line_max
    p = np.zeros(4, np.int32)
    pp, out = p.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(0)
    assert fn(pp, 0, 0, 4, C.byref(out)) == -1      # n < 1
    assert fn(pp, 4, -1, 4, C.byref(out)) == -1     # lo < 0
    assert fn(pp, 4, 1, 4, C.byref(out)) == -1      # lo + n > len
    assert fn(pp, 4, 0, 16385, C.byref(out)) == -1  # longer than the largest frame side
    assert fn(None, 4, 0, 4, C.byref(out)) == -1
    p[2] = -2
    assert fn(pp, 4, 0, 4, C.byref(out)) == -1


def test_norm_grows_with_either_argument():
    """what stop rules (a) and (b) rest on"""
    d = np.arange(0, 700)
    t = norm5(d[:, None], d[None, :])
    assert (np.diff(t, axis=0) > 0).all() and (np.diff(t, axis=1) > 0).all()
    assert (t == t.T).all()
    big = norm5(np.array([16384]), np.array([16384]))
    assert int(big[0]) < 2 ** 32
