"""The sample table of the ML-only grasp selection without a device (include/leafgrasp.h: lg_ml_sample_points_host, the code
lg_ml_rows_kernel and lg_ml_table_kernel run), against a NumPy restatement, bit for bit:

  order     np.where order of the set mask pixels (row-major)
  NTH       step = max(1, n // target), samples = pixels 0, step, 2 step, ... (grasp_point_selector.py:310-320), at most
            2 target - 1 of them
  GRID      the set pixels with x % stride == 0 and y % stride == 0; more than the table holds: *n = -(their number)
  border    scored = not (y < 16 or y >= H - 16 or x < 16 or x >= W - 16)   (:326-328)
  sums      sum x, sum y, area as exact integers

Frames 1 x 1, 33 x 70, 64 x 128, 96 x 136 (a last word of 8 bits), 130 x 257 and 1100 x 72 (more rows than one workgroup of the
device pass takes at a time); masks of area 0, 1, 99, 100, 101, 199, 200, 201, a random blob, a leaf inside the border band, one
crossing it, and a full frame; target 1, 7, 100; stride 1, 3, 8, 64."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402

lib = _lib.lib
NTH, GRID = _lib.LG_ML_SAMPLE_NTH, _lib.LG_ML_SAMPLE_GRID
SHAPES = [(1, 1), (33, 70), (64, 128), (96, 136), (130, 257), (1100, 72)]
AREAS = [0, 1, 99, 100, 101, 199, 200, 201]


def pack_bits(mask):
    """bit rows [H][WW] uint64: bit j of word w = pixel 64 w + j, bits past W zero"""
    H, W = mask.shape
    WW = (W + 63) // 64
    pad = np.zeros((H, WW * 64), np.uint8)
    pad[:, :W] = mask != 0
    return np.packbits(pad.reshape(H, WW, 64), axis=2, bitorder="little").view(np.uint64).reshape(H, WW).copy()


def sampling(mode, target=100, stride=8, max_samples=4096, chunk=0):
    return _lib.LgMlSampling(mode, target, stride, max_samples, chunk)


def host_table(mask, s, cap=None):
    H, W = mask.shape
    bits = pack_bits(mask)
    cap = s.max_samples if cap is None else cap
    xy = np.full((cap, 2), -7, np.int32)
    scored = np.full(cap, -7, np.int32)
    n = C.c_int32(-12345)
    sums = (C.c_int64 * 3)()
    rc = lib.lg_ml_sample_points_host(bits.ctypes.data, H, W, bits.shape[1], C.byref(s), xy.ctypes.data, scored.ctypes.data, cap,
                                      C.byref(n), sums)
    return rc, n.value, xy, scored, [int(v) for v in sums]


def numpy_table(mask, s, cap=None):
    """(n, xy [n, 2], scored [n], sums): the restatement"""
    H, W = mask.shape
    cap = s.max_samples if cap is None else min(cap, s.max_samples)
    ys, xs = np.where(mask != 0)
    n = len(ys)
    sums = [int(xs.astype(np.int64).sum()), int(ys.astype(np.int64).sum()), n]
    if s.mode == NTH:
        step = max(1, n // s.target)
        sx, sy = xs[::step], ys[::step]
    else:
        keep = (xs % s.stride == 0) & (ys % s.stride == 0)
        sx, sy = xs[keep], ys[keep]
        if len(sx) > cap:
            return -len(sx), None, None, sums
    scored = ~((sy < 16) | (sy >= H - 16) | (sx < 16) | (sx >= W - 16))
    return len(sx), np.stack([sx, sy], 1).astype(np.int32).reshape(-1, 2), scored.astype(np.int32), sums


def masks_for(H, W):
    """name -> mask of one frame"""
    rng = np.random.default_rng(1000 * H + W)
    out = {}
    for a in AREAS:   # `a` pixels scattered over the frame (as many as the frame holds)
        m = np.zeros(H * W, np.uint8)
        m[rng.choice(H * W, size=min(a, H * W), replace=False)] = 1
        out[f"area{a}"] = m.reshape(H, W)
    yy, xx = np.mgrid[:H, :W]
    cy, cx = H * 0.55, W * 0.45
    blob = ((yy - cy) / max(H * 0.3, 1)) ** 2 + ((xx - cx) / max(W * 0.35, 1)) ** 2 <= 1.0
    out["blob"] = (blob & (rng.random((H, W)) < 0.9)).astype(np.uint8)
    band = np.zeros((H, W), np.uint8)
    band[: min(H, 12), : min(W, 40)] = 1                       # wholly inside the 16-pixel border band
    out["in_band"] = band
    cross = np.zeros((H, W), np.uint8)
    cross[min(H - 1, 5): min(H, 40), min(W - 1, 9): min(W, 60)] = 1   # crosses it (where the frame has an interior)
    out["crossing"] = cross
    out["full"] = np.ones((H, W), np.uint8)
    return out


def check(mask, s, cap=None):
    rc, n, xy, scored, sums = host_table(mask, s, cap)
    assert rc == 0
    en, exy, esc, esums = numpy_table(mask, s, cap)
    assert sums == esums
    assert n == en
    if en > 0:
        assert np.array_equal(xy[:en], exy)
        assert np.array_equal(scored[:en], esc)
    k = max(en, 0)
    assert (xy[k:] == -7).all() and (scored[k:] == -7).all()   # nothing is written past the samples
    return en


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nth_equals_numpy(shape):
    for name, mask in masks_for(*shape).items():
        area = int(mask.sum())
        for target in (1, 7, 100):
            n = check(mask, sampling(NTH, target=target))
            assert n <= 2 * target - 1, (name, target)        # the count bound
            assert (n == 0) == (area == 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_equals_numpy(shape):
    for name, mask in masks_for(*shape).items():
        for stride in (1, 3, 8, 64):
            check(mask, sampling(GRID, stride=stride, max_samples=65536))


def test_step_rule_at_the_thresholds():
    """target 100: areas 99, 100, 101, 199 take every pixel, 200 and 201 every second one"""
    for a, en in [(0, 0), (1, 1), (99, 99), (100, 100), (101, 101), (199, 199), (200, 100), (201, 101)]:
        mask = np.zeros((64, 128), np.uint8)
        mask.reshape(-1)[np.arange(a) * 37 % (64 * 128)] = 1
        assert int(mask.sum()) == a
        assert check(mask, sampling(NTH, target=100)) == en


def test_grid_overflow_code():
    mask = np.ones((96, 136), np.uint8)
    need = len(range(0, 96, 8)) * len(range(0, 136, 8))   # 12 * 17
    for cap, ms in [(need - 1, 4096), (4096, need - 1), (1, 1)]:
        rc, n, xy, scored, sums = host_table(mask, sampling(GRID, stride=8, max_samples=ms), cap)
        assert rc == 0 and n == -need
        assert (xy == -7).all() and (scored == -7).all()
        assert sums == [int(np.arange(136).sum()) * 96, int(np.arange(96).sum()) * 136, 96 * 136]
    assert check(mask, sampling(GRID, stride=8, max_samples=need), need) == need   # exactly full is no overflow


def test_outputs_may_be_null():
    mask = masks_for(64, 128)["blob"]
    bits = pack_bits(mask)
    s = sampling(NTH, target=7)
    n = C.c_int32()
    assert lib.lg_ml_sample_points_host(bits.ctypes.data, 64, 128, 2, C.byref(s), None, None, 4096, C.byref(n), None) == 0
    assert n.value == numpy_table(mask, s)[0]


def test_invalid_arguments():
    mask = masks_for(64, 128)["blob"]
    bits = pack_bits(mask)
    xy, sc, n = np.zeros((4096, 2), np.int32), np.zeros(4096, np.int32), C.c_int32()

    def call(s, bits_ptr=bits.ctypes.data, H=64, W=128, WW=2, cap=4096, n_ref=C.byref(n)):
        return lib.lg_ml_sample_points_host(bits_ptr, H, W, WW, C.byref(s) if s is not None else None, xy.ctypes.data, sc.ctypes.data,
                                            cap, n_ref, None)

    assert call(sampling(NTH)) == 0
    bad = _lib.LG_ERR_INVALID
    assert call(None) == bad
    assert call(sampling(NTH), bits_ptr=None) == bad
    assert call(sampling(NTH), n_ref=None) == bad
    assert call(sampling(NTH), H=0) == bad
    assert call(sampling(NTH), WW=3) == bad
    assert call(sampling(NTH), cap=0) == bad
    assert call(sampling(2)) == bad
    assert call(sampling(NTH, target=0)) == bad
    assert call(sampling(NTH, target=100, max_samples=198)) == bad    # 2 target - 1 = 199 samples must fit
    assert call(sampling(NTH, target=100), cap=198) == bad
    assert call(sampling(NTH, target=100, max_samples=199), cap=199) == 0
    assert call(sampling(GRID, stride=0)) == bad
    assert call(sampling(GRID, stride=65)) == bad
    assert call(sampling(GRID, max_samples=0)) == bad
    assert call(sampling(GRID, max_samples=65537)) == bad
    assert call(sampling(GRID, chunk=-1)) == bad


def test_structs_and_defaults():
    assert C.sizeof(_lib.LgMlSample) == 20 and C.sizeof(_lib.LgMlSampling) == 20
    s = _lib.LgMlSampling()
    lib.lg_default_ml_sampling(C.byref(s))
    assert (s.mode, s.target, s.stride, s.max_samples, s.chunk) == (NTH, 100, 8, 4096, 0)
