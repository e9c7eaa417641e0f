"""lg_tail_lane_plan, the pure rule behind the tail lanes of lg_select_grasp ("Tail in lanes"), against a
three-line restatement: no device, no handle.

The automatic setting (requested = 0) is a measured pair -- so many lanes from so many frames on -- that the library owns
(LG_TAIL_LANES_AUTO, LG_TAIL_LANES_MIN_B in lg_select.hip).  The test reads the pair back through the rule itself, holds it to
what the header promises of any such pair (one threshold, 1 .. 4 lanes above it, one lane below) and restates the rest."""
import ctypes as C

import pytest

from leafgrasp_amd._lib import LG_ERR_INVALID, LG_OK, lib

BATCHES = tuple(range(1, 10)) + (255, 256, 257)


def plan(B, requested, eligible):
    lanes, sb = C.c_int32(-1), C.c_int32(-1)
    rc = lib.lg_tail_lane_plan(B, requested, 1 if eligible else 0, C.byref(lanes), C.byref(sb))
    assert rc == LG_OK, (B, requested, eligible, rc)
    return int(lanes.value), int(sb.value)


def automatic():
    """(lanes, first batch size that takes them) of the automatic rule, found by asking it; (1, None) when it never engages."""
    got = [plan(B, 0, True)[0] for B in range(1, 4097)]
    if max(got) == 1:
        return 1, None
    b_min = next(B for B, n in zip(range(1, 4097), got) if n > 1)
    return got[b_min - 1], b_min


def test_the_automatic_rule_is_one_threshold():
    lanes, b_min = automatic()
    print(f"automatic rule: {lanes} lanes from {b_min} frames on")
    assert 1 <= lanes <= 4
    for B in range(1, 4097):
        want = lanes if b_min is not None and B >= b_min else 1
        assert plan(B, 0, True)[0] == -(-B // -(-B // min(want, B))), B


@pytest.mark.parametrize("eligible", (True, False))
@pytest.mark.parametrize("requested", range(5))
def test_plan_against_its_restatement(requested, eligible):
    auto_lanes, b_min = automatic()
    for B in BATCHES:
        want = requested or (auto_lanes if b_min is not None and B >= b_min else 1)
        want = min(want if eligible else 1, B)                  # a lane never holds fewer than one frame
        sb = -(-B // want)                                      # frames per lane
        lanes = -(-B // sb)                                     # lanes that hold a frame
        assert plan(B, requested, eligible) == (lanes, sb), (B, requested, eligible)
        # the lanes cover [0, B) without gap or overlap, and none is empty
        ranges = [(k * sb, min((k + 1) * sb, B)) for k in range(lanes)]
        assert ranges[0][0] == 0 and ranges[-1][1] == B
        assert all(a < b for a, b in ranges) and all(ranges[i][1] == ranges[i + 1][0] for i in range(lanes - 1))
        assert lanes <= want and (eligible or lanes == 1)


def test_bad_arguments():
    lanes, sb = C.c_int32(), C.c_int32()
    for B, req in ((0, 0), (-1, 2), (4, -1), (4, 5)):
        assert lib.lg_tail_lane_plan(B, req, 1, C.byref(lanes), C.byref(sb)) == LG_ERR_INVALID
    assert lib.lg_tail_lane_plan(4, 2, 1, None, C.byref(sb)) == LG_ERR_INVALID
    assert lib.lg_tail_lane_plan(4, 2, 1, C.byref(lanes), None) == LG_ERR_INVALID
