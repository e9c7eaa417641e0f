"""The experiment switches as the library parses them (csrc/lg_options.cpp), without a device: lg_options_text runs the parser
of a handle (0), a model (1) or a trainer (2) on the environment as it is and prints one NAME=value line per switch.  The
tables below are written by hand from the parsing code the switches had where they used to be read (lg_create, lg_orient_ensure,
lg_launch_final, lg_cnn_load, lg_train_create) -- defaults, clamps and accepted sets -- not produced by the parser."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from leafgrasp_amd import _lib  # noqa: E402

HANDLE, MODEL, TRAINER = 0, 1, 2


def cpus():
    return len(os.sched_getaffinity(0))


def host_threads(ranks=1):
    """this process's share of the CPUs it may run on, at most 16, at least 1"""
    return max(1, min(cpus() // ranks, 16))


DEFAULTS = {
    HANDLE: dict(LG_HOST_THREADS=None, LG_SUBBATCH=0, LG_TRACE=0, LG_NO_SKIP=0, LG_FINAL_NEAR=1, LG_FINAL_PERSIST=-1, LG_FINAL_TPW=-1,
                 LG_HOST_ORIENT=0, LG_CNN_PRUNE=1, LG_DEFER_PLANES=1, LG_DT_SEARCH=2, LG_DT_SEARCH_ALGO=0, LG_DT_BAND_P=16,
                 LG_DT_BAND_E=4, LG_SIDE_TAIL=1, LG_STEM_ALGO=1, LG_DIRECT_HOST=1, LG_ORIENT_CAP=16384, LG_ORIENT_FAIL=0),
    MODEL: dict(LG_CNN_F23=0, LG_CNN_WINO_MASK=0x3f),
    TRAINER: dict(LG_TRAIN_GRAPH=0, LG_TRAIN_STREAMS=1, LG_TRAIN_CONV_SMALL=256, LG_TRAIN_CONV_SPLIT=256),
}

RETIRED = ("LG_DT_E", "LG_DT_SEARCH_BUDGET", "LG_DT_SEARCH_G", "LG_NT_STORES", "LG_PLANE_SKEW", "LG_EXPORT_MEMCPY", "LG_LEAF_GX",
           "LG_CNN_CUS", "LG_LEAF_ABLATE")

# every name any parser looks at: the tests start from none of them set
ALL_NAMES = sorted({n for d in DEFAULTS.values() for n in d} | {"LOCAL_WORLD_SIZE", "LG_CNN_DIRECT"} | set(RETIRED))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for n in ALL_NAMES:
        monkeypatch.delenv(n, raising=False)


def text(which):
    import ctypes as C

    buf = C.create_string_buffer(4096)
    n = _lib.lib.lg_options_text(which, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def parsed(which):
    out = {}
    for ln in text(which).splitlines():
        k, v = ln.split("=")
        assert k not in out
        out[k] = int(v)
    return out


def want(which, **changed):
    d = dict(DEFAULTS[which])
    if which == HANDLE:
        d["LG_HOST_THREADS"] = host_threads()
    assert set(changed) <= set(d)
    d.update(changed)
    return d


def test_defaults_with_nothing_set():
    for which in (HANDLE, MODEL, TRAINER):
        assert parsed(which) == want(which), which
        assert text(which).endswith("\n") and list(parsed(which)) == list(DEFAULTS[which])   # one line per switch, in order


def one_of(accepted, default, others):
    """a switch that takes a value of `accepted` and keeps its default for any other"""
    return [(str(v), v) for v in accepted] + [(str(v), default) for v in others] + [("abc", 0 if 0 in accepted else default)]


def on_unless_zero():
    return [("0", 0), ("1", 1), ("2", 1), ("-1", 1), ("abc", 0), ("", 0)]


def presence():
    return [("1", 1), ("0", 1), ("", 1), ("abc", 1)]


# name -> [(text, value its own line then shows)]
HANDLE_CASES = {
    "LG_HOST_THREADS": [("1", 1), ("5", 5), ("64", 64), ("0", 1), ("-3", 1), ("abc", 1)],                    # max(1, n), no upper end
    "LG_SUBBATCH": [("1", 1), ("4", 4), ("64", 64), ("0", 1), ("-2", 1), ("abc", 1)],                        # max(1, n)
    "LG_TRACE": presence(),
    "LG_NO_SKIP": [("1", 1), ("2", 2), ("3", 3), ("0", 1), ("-1", 1), ("4", 0), ("5", 1), ("7", 3), ("abc", 1)],   # max(1, n) & 3
    "LG_FINAL_NEAR": [("0", 0), ("1", 1), ("2", 2), ("8", 8), ("64", 64), ("65", 64), ("-1", 0), ("abc", 0)],        # 0..64
    "LG_HOST_ORIENT": presence(),
    "LG_CNN_PRUNE": on_unless_zero(),
    "LG_DEFER_PLANES": on_unless_zero(),
    "LG_DT_SEARCH": [("0", 0), ("1", 1), ("2", 2), ("3", 2), ("-1", 0), ("abc", 0)],                         # 0..2
    "LG_DT_SEARCH_ALGO": one_of((0, 1, 5, 6), 0, (-1, 2, 3, 4, 7)),
    "LG_DT_BAND_P": one_of((12, 16, 24, 32), 16, (0, 8, 11, 13, 31, 33)),
    "LG_DT_BAND_E": one_of((2, 4), 4, (0, 1, 3, 5, 8)),
    "LG_SIDE_TAIL": [("0", 0), ("1", 1), ("2", 2), ("3", 2), ("-1", 0), ("abc", 0)],                         # 0..2
    "LG_STEM_ALGO": on_unless_zero(),
    "LG_DIRECT_HOST": on_unless_zero(),
    "LG_ORIENT_CAP": [("16", 16), ("17", 17), ("64", 64), ("320", 320), ("16384", 16384), ("15", 16), ("0", 16), ("-5", 16),
                      ("16385", 16384), ("abc", 16)],                                                          # 16..16384
    "LG_ORIENT_FAIL": presence(),
}


@pytest.mark.parametrize("name", list(HANDLE_CASES))
def test_handle_switch(monkeypatch, name):
    for value, shown in HANDLE_CASES[name]:
        monkeypatch.setenv(name, value)
        assert parsed(HANDLE) == want(HANDLE, **{name: shown}), (name, value)


@pytest.mark.parametrize("name", ["LG_FINAL_PERSIST", "LG_FINAL_TPW"])
def test_launch_shape_switches_turn_the_near_launch_off(monkeypatch, name):
    """the number as written (a negative one leaves the launch form alone, as when unset); being set is what clears LG_FINAL_NEAR"""
    for value, shown in [("0", 0), ("3", 3), ("4", 4), ("8", 8), ("-1", -1), ("-2", -2), ("abc", 0), ("", 0)]:
        monkeypatch.setenv(name, value)
        assert parsed(HANDLE) == want(HANDLE, **{name: shown, "LG_FINAL_NEAR": 0}), (name, value)
        monkeypatch.setenv("LG_FINAL_NEAR", "4")   # whatever LG_FINAL_NEAR asks for
        assert parsed(HANDLE) == want(HANDLE, **{name: shown, "LG_FINAL_NEAR": 0}), (name, value)
        monkeypatch.delenv("LG_FINAL_NEAR")
    monkeypatch.setenv("LG_FINAL_PERSIST", "3")
    monkeypatch.setenv("LG_FINAL_TPW", "4")
    assert parsed(HANDLE) == want(HANDLE, LG_FINAL_PERSIST=3, LG_FINAL_TPW=4, LG_FINAL_NEAR=0)


def test_ranks_share_the_host_threads(monkeypatch):
    for value, ranks in [("1", 1), ("2", 2), ("8", 8), ("100000", 100000), ("0", 1), ("-4", 1), ("abc", 1)]:
        monkeypatch.setenv("LOCAL_WORLD_SIZE", value)
        assert parsed(HANDLE) == want(HANDLE, LG_HOST_THREADS=host_threads(ranks)), value
    monkeypatch.setenv("LG_HOST_THREADS", "3")   # the explicit number wins
    assert parsed(HANDLE) == want(HANDLE, LG_HOST_THREADS=3)


def test_model_switches(monkeypatch):
    for value in ("1", "0", ""):
        monkeypatch.setenv("LG_CNN_F23", value)
        assert parsed(MODEL) == want(MODEL, LG_CNN_F23=1), value
    monkeypatch.delenv("LG_CNN_F23")
    for value in ("1", "0", ""):
        monkeypatch.setenv("LG_CNN_DIRECT", value)
        assert parsed(MODEL) == want(MODEL, LG_CNN_WINO_MASK=0), value
    masks = [("0", 0), ("1", 1), ("21", 21), ("62", 62), ("63", 63), ("64", 0), ("65", 1), ("127", 63), ("-1", 63), ("abc", 0)]   # n & 0x3f
    for value, shown in masks:   # ... and the mask takes precedence over LG_CNN_DIRECT
        monkeypatch.setenv("LG_CNN_WINO_MASK", value)
        assert parsed(MODEL) == want(MODEL, LG_CNN_WINO_MASK=shown), value
    monkeypatch.delenv("LG_CNN_DIRECT")
    for value, shown in masks:
        monkeypatch.setenv("LG_CNN_WINO_MASK", value)
        assert parsed(MODEL) == want(MODEL, LG_CNN_WINO_MASK=shown), value


TRAINER_CASES = {
    "LG_TRAIN_GRAPH": on_unless_zero(),
    "LG_TRAIN_STREAMS": [("2", 2), ("1", 1), ("0", 1), ("3", 1), ("-2", 1), ("abc", 1), ("", 1)],   # the second stream at 2 only
    "LG_TRAIN_CONV_SMALL": [("0", 0), ("1", 1), ("256", 256), ("1000000", 1000000), ("-1", -1), ("abc", 0)],   # as written
    "LG_TRAIN_CONV_SPLIT": [("0", 0), ("1", 1), ("256", 256), ("1000000", 1000000), ("-1", -1), ("abc", 0)],
}


@pytest.mark.parametrize("name", list(TRAINER_CASES))
def test_trainer_switch(monkeypatch, name):
    for value, shown in TRAINER_CASES[name]:
        monkeypatch.setenv(name, value)
        assert parsed(TRAINER) == want(TRAINER, **{name: shown}), (name, value)


def test_a_switch_changes_its_own_object_only(monkeypatch):
    for name in list(HANDLE_CASES) + ["LG_FINAL_PERSIST", "LG_FINAL_TPW", "LOCAL_WORLD_SIZE"]:
        monkeypatch.setenv(name, "2")
    assert parsed(MODEL) == want(MODEL) and parsed(TRAINER) == want(TRAINER)
    for name in TRAINER_CASES:
        monkeypatch.setenv(name, "2")
    assert parsed(MODEL) == want(MODEL)
    for name in ALL_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name in list(TRAINER_CASES) + ["LG_CNN_F23", "LG_CNN_DIRECT", "LG_CNN_WINO_MASK"]:
        monkeypatch.setenv(name, "2")
    assert parsed(HANDLE) == want(HANDLE)


@pytest.mark.parametrize("name", RETIRED)
def test_retired_names_change_nothing(monkeypatch, name):
    for value in ("1", "8", "64"):
        monkeypatch.setenv(name, value)
        for which in (HANDLE, MODEL, TRAINER):
            assert parsed(which) == want(which), (name, value, which)


def test_text_buffer_and_arguments():
    import ctypes as C

    full = text(HANDLE)
    buf = C.create_string_buffer(16)
    assert _lib.lib.lg_options_text(HANDLE, buf, len(buf)) == len(full)   # the whole length, the text cut to fit and terminated
    assert buf.value.decode() == full[:15]
    assert _lib.lib.lg_options_text(3, buf, len(buf)) == -1 and _lib.lib.lg_options_text(-1, buf, len(buf)) == -1
    assert _lib.lib.lg_options_text(HANDLE, None, 16) == -1 and _lib.lib.lg_options_text(HANDLE, buf, 0) == -1
