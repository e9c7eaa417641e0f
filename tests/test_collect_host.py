"""CPU tests (no GPU) of the collecting selector's host twins (include/leafgrasp.h, lg_select_grasp_collect): the ellipse erosion
on bit rows against the erosion composed from the oracle's dilation, the closed form of the tip penalty's 5 x 5 transform against
the oracle's 16.16 field, the defaults, every refusal, and the struct's size."""
import ctypes as C

import numpy as np
import pytest

from leafgrasp_amd import _lib
from oracle import lg_oracle as O
from tests import collect_ref as CR
from tests.collector_cases import pack_bits

lib = _lib.lib
H = 72


def _erode_words(mask, k, iterations):
    Hh, W = mask.shape
    WW = (W + 63) // 64
    bits = pack_bits(mask)
    if W % 64:
        bits[:, -1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (W % 64)) - 1))   # junk past W is ignored
    out = np.zeros((Hh, WW), np.uint64)
    rc = lib.lg_erode_words_host(bits.ctypes.data, Hh, W, WW, k, iterations, out.ctypes.data)
    assert rc == 0
    return out


@pytest.mark.parametrize("W", [63, 64, 65, 128, 129])
@pytest.mark.parametrize("k,iterations", [(3, 1), (3, 2), (5, 2), (15, 1), (21, 1), (21, 2), (63, 1)])
def test_erode_words_host_is_the_composed_erosion(W, k, iterations):
    for name, mask in CR.erosion_masks(H, W).items():
        exp = CR.erode(mask, k, iterations)
        got = _erode_words(mask, k, iterations)
        np.testing.assert_array_equal(got, pack_bits(exp), err_msg=f"{name} W={W} k={k} x{iterations}")
        if name == "full":
            assert exp.all()                   # the frame border does not erode
        if name == "ellipse" and k <= 21:
            assert 0 < exp.sum() < mask.sum()   # something erodes, something stays


def test_erosion_passes_do_not_fold_into_one_kernel():
    """two passes of the 21 ellipse are not one pass of a 41 ellipse (the ellipse is no rectangle)"""
    mask = CR.erosion_masks(120, 160)["ellipse"]
    assert not np.array_equal(CR.erode(mask, 21, 2), CR.erode(mask, 41, 1))


def test_zero_iterations_and_size_one_leave_the_mask():
    mask = CR.erosion_masks(H, 129)["hole"]
    np.testing.assert_array_equal(_erode_words(mask, 21, 0), pack_bits(mask))
    np.testing.assert_array_equal(_erode_words(mask, 1, 3), pack_bits(mask))


@pytest.mark.parametrize("init0", [O.INIT_DIST0, 2 ** 31 - 1])
@pytest.mark.parametrize("shape", [(200, 264), (121, 167), (8, 8), (9, 40)])
def test_tip_closed_form_is_the_oracles_transform(init0, shape):
    Hh, W = shape
    _, fix = CR.tip_field_as_written(Hh, W, init0)
    got = np.zeros((Hh, W), np.uint32)
    mx = C.c_uint32()
    assert lib.lg_tip_fix_host(Hh, W, init0, got.ctypes.data, C.byref(mx)) == 0
    np.testing.assert_array_equal(got, fix)
    assert mx.value == int(fix.max())


def test_default_collect_params():
    p = _lib.LgCollectParams()
    lib.lg_default_collect_params(C.byref(p))
    assert (p.erosion_kernel_size, p.erosion_iterations, p.tip_se, p.tip_aware) == (21, 2, 15, 0)
    assert round(p.w_tip, 6) == 0.1
    assert C.sizeof(_lib.LgCollectParams) == 5 * 4
    assert lib.lg_collect_params_check(None, None) == 0
    assert lib.lg_collect_params_check(C.byref(_lib.default_params()), C.byref(p)) == 0


@pytest.mark.parametrize("field,value,code", [
    ("erosion_kernel_size", 20, _lib.LG_ERR_UNSUPPORTED), ("erosion_kernel_size", 0, _lib.LG_ERR_UNSUPPORTED),
    ("erosion_kernel_size", 65, _lib.LG_ERR_UNSUPPORTED), ("erosion_kernel_size", -3, _lib.LG_ERR_UNSUPPORTED),
    ("erosion_iterations", -1, _lib.LG_ERR_UNSUPPORTED), ("erosion_iterations", 9, _lib.LG_ERR_UNSUPPORTED),
    ("tip_aware", 2, _lib.LG_ERR_INVALID), ("tip_aware", -1, _lib.LG_ERR_INVALID),
    ("tip_aware", 1, _lib.LG_ERR_UNSUPPORTED),   # the opt-in transform of the tip area is not built
    ("erosion_kernel_size", 63, 0), ("erosion_kernel_size", 1, 0), ("erosion_iterations", 0, 0), ("erosion_iterations", 8, 0),
    ("tip_se", 14, 0), ("tip_se", 1, 0),         # read only when tip_aware
])
def test_collect_params_refusals(field, value, code):
    p = _lib.LgCollectParams()
    lib.lg_default_collect_params(C.byref(p))
    setattr(p, field, value)
    assert lib.lg_collect_params_check(None, C.byref(p)) == code


@pytest.mark.parametrize("tip_se", [2, 14, 1, 65])
def test_tip_se_is_checked_when_tip_aware(tip_se):
    p = _lib.LgCollectParams()
    lib.lg_default_collect_params(C.byref(p))
    p.tip_aware, p.tip_se = 1, tip_se
    assert lib.lg_collect_params_check(None, C.byref(p)) == _lib.LG_ERR_UNSUPPORTED


def test_label_aware_is_refused():
    q = _lib.default_params()
    q.label_aware = 1
    assert lib.lg_collect_params_check(C.byref(q), None) == _lib.LG_ERR_INVALID


def test_erode_words_host_refuses_bad_arguments():
    bits = np.zeros((8, 1), np.uint64)
    out = np.zeros((8, 1), np.uint64)
    f = lib.lg_erode_words_host
    assert f(bits.ctypes.data, 8, 8, 1, 4, 1, out.ctypes.data) == _lib.LG_ERR_UNSUPPORTED
    assert f(bits.ctypes.data, 8, 8, 1, 65, 1, out.ctypes.data) == _lib.LG_ERR_UNSUPPORTED
    assert f(bits.ctypes.data, 8, 8, 1, 3, 9, out.ctypes.data) == _lib.LG_ERR_UNSUPPORTED
    assert f(bits.ctypes.data, 8, 8, 2, 3, 1, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert f(None, 8, 8, 1, 3, 1, out.ctypes.data) == _lib.LG_ERR_INVALID
    assert lib.lg_tip_fix_host(8, 8, 12345, out.ctypes.data, None) == _lib.LG_ERR_INVALID


def test_composed_scene_has_the_figures_the_gpu_tests_rely_on():
    """seed 1 of the whole-entry scene, composed here: the sizes and the margin the GPU test's pixel assertion stands on"""
    mask, depth, P = CR.entry_scene(1)
    r = CR.compose(mask, depth, P)
    assert 16000 < int(r["safe"].sum()) < 18000 and 8000 < int(r["valid"].sum()) < 9500
    assert r["by_argmax"] and 0.9 < r["best_score"] < 1.0
    assert r["valid"][r["point"][1], r["point"][0]]
    tip = r["scores"][CR.TIP_KEY]
    assert 0.0 <= tip.min() and 0.005 < tip.max() < 0.03 and not tip[r["safe"] == 0].any()   # a ramp of a few per cent
