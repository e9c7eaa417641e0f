"""The plan of the pruned CNN pass as tests/cnn_plan.py restates it (device_plan: grid from the host's bound B * top_k, items
from the device's survivor count), without a device: the batches tests/test_gpu_cnn_prune_regimes.py runs reach every plan
class of every layer the picker finds, on the MI355X's 256 CUs and on 304; the compositions give the counts they claim."""
import pytest

from tests import cnn_plan as C

LAYERS = C.model_layers((64, 128, 256))


def test_device_plan_by_hand():
    # 256 -> 256 channels at 8 x 8 (8 patches per tile block, 4 channel blocks), 256 CUs = 32 workgroups per XCD
    ci, co, wi = LAYERS[5]
    assert (ci, co, wi) == (256, 256, 8)
    assert C.device_plan(ci, co, wi, 400, 400, 256) == (1, 0, 0)       # 50 tile blocks: 7 x 4 = 28 items, grid shrunk to them
    assert C.device_plan(ci, co, wi, 400, 65, 256) == (0, 8, 160)      # 9 tile blocks: 2 x 4 items on 28 workgroups per XCD
    assert C.device_plan(ci, co, wi, 400, 64, 256) == (0, 4, 192)      # 8 tile blocks: one per XCD
    assert C.device_plan(ci, co, wi, 400, 0, 256) == (0, 0, 224)
    assert C.device_plan(ci, co, wi, 8192, 8192, 256) == (16, 0, 0)    # 1024 tile blocks: 128 x 4 items on 32
    assert C.device_plan(ci, co, wi, 8192, 920, 256) == (1, 28, 0)     # the headline's count: 115 tile blocks, 15 x 4 items
    # 12 -> 64 at 32 x 32: two tile blocks per patch
    ci, co, wi = LAYERS[0]
    assert C.device_plan(ci, co, wi, 20, 1, 256) == (0, 1, 32)         # host: 40 tile blocks, 5 workgroups per XCD
    assert C.device_plan(ci, co, wi, 640, 115, 256) == (0, 29, 24)
    assert C.device_plan(ci, co, wi, 640, 200, 256) == (1, 18, 0)


def test_slices():
    assert C.device_slices(8320, 100) == [(8192, 100), (128, 0)]
    assert C.device_slices(8320, 8301) == [(8192, 8192), (128, 109)]
    assert C.device_slices(8256, 8193) == [(8192, 8192), (64, 1)]
    assert C.device_slices(8420, 8192) == [(8192, 8192), (228, 0)]
    assert C.device_slices(60, 60) == [(60, 60)]


def test_compose():
    for nh in range(1, 400):
        for nd in range(nh + 1):
            c = C.compose(nh, nd)
            if c is not None:
                b, k, e = c
                assert b * k == nh and C.survivors_of(b, k, e) == nd and 0 <= e <= b and 1 <= k <= 64
    assert C.compose(8256, 8193) == (129, 64, 128) and C.compose(8320, 8301) == (416, 20, 415)
    assert C.compose(7, 3) is None
    for name, b, k, e in C.EXTRA_BATCHES:
        assert name in ("none", "one", "all", "all, odd") or int(name) == C.survivors_of(b, k, e)
    by = {n: C.survivors_of(b, k, e) for n, b, k, e in C.EXTRA_BATCHES}
    assert by["none"] == 0 and by["one"] == 1 and by["all"] == 60 and by["all, odd"] == 21
    assert by["17"] % 2 == 1 and by["57"] % 8 and by["8301"] - 8192 > 32 and (by["8301"] - 8192) % 8


@pytest.mark.parametrize("num_cu", [256, 304])
def test_batches_reach_every_class(num_cu):
    first = C.pick_device_pairs(LAYERS, num_cu)
    batches = C.prune_batches(LAYERS, num_cu)
    print()
    print(C.device_table(LAYERS, batches, num_cu))
    hit = set()
    for _, b, k, e in batches:
        hit |= C.device_classes(LAYERS, b * k, C.survivors_of(b, k, e), num_cu)
    for (li, c), (nh, nd) in first.items():
        print(f"L{li} {C.device_class_name(c):24s} first at n_host {nh:4d} n_dev {nd:4d}: {'hit' if (li, c) in hit else 'MISSED'}")
        assert nh <= 1300
    assert set(first) <= hit
    # every layer: no item, items on some workgroups, full rounds alone, full rounds and a left-over round
    classes = {(False, False, True, True), (False, True, True, False), (True, False, False, False), (True, True, False, False)}
    assert {c for _, c in first} == classes
    assert set(first) == {(li, c) for li in range(len(LAYERS)) for c in classes}
    # the second slice of a pruned pass: on nothing, on one patch, and on a count that fills no tile block of any layer
    for nd, second in ((8192, 0), (8193, 1), (8301, 109)):
        bb, kk, ee = next(t[1:] for t in batches if t[0] == str(nd))
        assert C.survivors_of(bb, kk, ee) == nd and C.device_slices(bb * kk, nd)[1][1] == second
