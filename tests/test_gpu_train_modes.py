"""One trainer handle through a sequence of steps of different batch sizes, mask sources and hyper-parameters, and the two
opt-in execution modes of lg_train_step: LG_TRAIN_GRAPH=1 (the step replayed as a captured graph, keyed on (N, mask source,
apply_update)) and LG_TRAIN_STREAMS=2 (backward-weights on a second stream, dX double-buffered behind event fences).  Both
switches are read at lg_train_create.  Neither mode changes the order of any sum, so every step must equal the default
mode's bit for bit.  The two switches are never set on one trainer."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import synthetic_inputs as S  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402
from tests.test_gpu_train import compare_step, make_trainer, random_masks  # noqa: E402
from tests.train_steps import assert_same_outputs, assert_same_state, load_from_snapshot, snapshot  # noqa: E402

MODELS = [("spatial", (32, 64, 128)), ("spatial", (64, 128, 256))]
MODEL_IDS = ["lightweight", "standard"]
SEED = 42
# (N, masks given by the host?, apply_update, change made before the step)
SEQUENCE = [(16, True, True, None), (13, False, True, None), (2, True, True, None), (16, True, False, None),
            (16, True, True, "halve_lr"), (13, False, True, "pos_weight_0.5"), (16, False, True, None), (2, False, True, None)]
ENV = {"default": {}, "graph": {"LG_TRAIN_GRAPH": "1"}, "streams": {"LG_TRAIN_STREAMS": "2"}}


def trainer_in_mode(monkeypatch, mode, att, filt, max_batch, **kw):
    for k, v in ENV[mode].items():
        monkeypatch.setenv(k, v)
    tr = make_trainer(att, filt, max_batch, seed=SEED, **kw)
    for k in ENV[mode]:
        monkeypatch.delenv(k)
    return tr


def start_state(att, filt):
    return {k: torch.from_numpy(v) for k, v in S.cnn_closed_form_params(seed=12, attention_type=att, filters=filt).items()}


def step_inputs(filt, i, n, given):
    x = S.synthetic_patches(n, seed=80 + i)
    y = ((np.arange(n) + i) % 3 == 0).astype(np.float32)
    return x, y, (random_masks(filt, n, 90 + i) if given else None)


def change(tr, what):
    if what == "halve_lr":
        tr.lr = tr.lr * 0.5
    elif what == "pos_weight_0.5":
        tr.hp.pos_weight = 0.5
    else:
        assert what is None


def run_sequence(tr, filt, before_step=None):
    """Returns [(outputs, snapshot after the step)] of SEQUENCE.  before_step(i, tr, step arguments) runs in front of step i."""
    rec = []
    for i, (n, given, upd, what) in enumerate(SEQUENCE):
        change(tr, what)
        x, y, mk = step_inputs(filt, i, n, given)
        if before_step:
            before_step(i, tr, (x, y, mk, upd))
        out = tr.train_step(x, y, masks=mk, apply_update=upd, return_logits=True)
        rec.append((out, snapshot(tr)))
    return rec


@functools.lru_cache(maxsize=None)
def default_mode_sequence(att, filt):
    """The sequence in the default mode (one stream, plain launches): computed once per model, never modified."""
    import os
    assert "LG_TRAIN_GRAPH" not in os.environ and "LG_TRAIN_STREAMS" not in os.environ
    tr = make_trainer(att, filt, 16, seed=SEED)
    tr.load_state_dict(start_state(att, filt))
    return run_sequence(tr, filt)


@pytest.mark.parametrize("att,filt", MODELS, ids=MODEL_IDS)
def test_sequence_every_step_equals_a_fresh_trainer(att, filt):
    """Before every step the full state is read; a FRESH trainer loaded with it performs the same step; outputs and the
    state after it are bit-equal.  Catches anything a step of another N leaves behind (masks laid out [layer][N][width],
    BatchNorm and backward-weights partials sized by N) and a hyper-parameter that does not reach the device."""
    fresh = []

    def before(i, tr, args):
        x, y, mk, upd = args
        f = make_trainer(att, filt, 16, seed=SEED, lr=tr.hp.lr, pos_weight=tr.hp.pos_weight)
        load_from_snapshot(f, snapshot(tr))
        fresh.append((f.train_step(x, y, masks=mk, apply_update=upd, return_logits=True), snapshot(f)))

    tr = make_trainer(att, filt, 16, seed=SEED)
    tr.load_state_dict(start_state(att, filt))
    rec = run_sequence(tr, filt, before)
    steps = 0
    for i, ((out, st), (fout, fst)) in enumerate(zip(rec, fresh)):
        assert_same_outputs(out, fout, f"step {i + 1} {SEQUENCE[i]}")
        assert_same_state(st, fst, f"step {i + 1} {SEQUENCE[i]}")
        steps += int(SEQUENCE[i][2])
        assert st["step"] == steps
    # the sequence is the one the other modes are compared with
    for (out, st), (dout, dst) in zip(rec, default_mode_sequence(att, filt)):
        assert_same_outputs(out, dout, "second run of the sequence")
        assert_same_state(st, dst, "second run of the sequence")
    # the changes did something: halving lr and pos_weight = 0.5 both move the result of their step
    assert rec[4][1]["step"] == 4 and tr.hp.pos_weight == 0.5 and tr.hp.lr == pytest.approx(2.5e-4)


@pytest.mark.parametrize("mode", ["graph", "streams"])
@pytest.mark.parametrize("att,filt", MODELS, ids=MODEL_IDS)
def test_sequence_in_opt_in_mode_equals_default_mode(monkeypatch, att, filt, mode):
    """graph: every key (N, mask source, apply_update) of the sequence is captured where it first occurs; steps 5 and 6
    replay the graphs of steps 1 and 2 with another lr, pos_weight, step count and mask seed, none of which may be baked
    into the graph.  (This is the test that found the replayed memset node: the gradient memset of a step used to be
    captured with it, and every replay left ~1e18 in the conv-bias gradients that only the memset writes.)
    streams: the backward-weights branch and its fences at N = 2, 13, 16."""
    tr = trainer_in_mode(monkeypatch, mode, att, filt, 16)
    tr.load_state_dict(start_state(att, filt))
    rec = run_sequence(tr, filt)
    for i, ((out, st), (dout, dst)) in enumerate(zip(rec, default_mode_sequence(att, filt))):
        assert_same_outputs(out, dout, f"{mode} step {i + 1} {SEQUENCE[i]}")
        assert_same_state(st, dst, f"{mode} step {i + 1} {SEQUENCE[i]}")


def test_graph_replay_of_one_key_three_times(monkeypatch):
    """The same key (16, given masks, update) three times in a row with other inputs, masks and lr each time: one capture,
    two replays."""
    att, filt = MODELS[0]
    trs = [trainer_in_mode(monkeypatch, m, att, filt, 16) for m in ("default", "graph")]
    for tr in trs:
        tr.load_state_dict(start_state(att, filt))
    for i in range(3):
        x, y, mk = step_inputs(filt, 20 + i, 16, True)
        outs = []
        for tr in trs:
            tr.lr = 5e-4 / (i + 1)
            outs.append((tr.train_step(x, y, masks=mk, return_logits=True), snapshot(tr)))
        assert_same_outputs(outs[0][0], outs[1][0], f"replay {i}")
        assert_same_state(outs[0][1], outs[1][1], f"replay {i}")


@pytest.mark.parametrize("att,filt,n", [("spatial", (64, 128, 256), 128), ("spatial", (32, 64, 128), 258)],
                         ids=["standard-128", "lightweight-258"])
def test_second_stream_at_the_batches_it_is_meant_for(monkeypatch, att, filt, n):
    """N = 128 and N = 258: BatchNorm reductions in sample chunks, backward-weights in many pixel slices -- the work the
    second stream overlaps.  Bit-equal with the default mode, and both held against the oracle by compare_step."""
    seed = 43
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=seed)
    y = (np.random.default_rng(seed).random(n) < 0.4).astype(np.float32)
    mk = random_masks(filt, n, seed)
    ref = O.cnn_train_step(params, x, y, masks=mk)
    res = {}
    for mode in ("default", "streams"):
        tr = trainer_in_mode(monkeypatch, mode, att, filt, n)
        tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        out = tr.train_step(x, y, masks=mk, return_logits=True)
        compare_step(tr, ref, *out, tight=True)
        out2 = tr.train_step(x, y, masks=None, return_logits=True)      # a second step: fences and buffers reused
        res[mode] = (out, out2, snapshot(tr))
    assert_same_outputs(res["default"][0], res["streams"][0], "first step")
    assert_same_outputs(res["default"][1], res["streams"][1], "second step")
    assert_same_state(res["default"][2], res["streams"][2], "after two steps")
