"""GPU tests of the trainer -> inference hand-off on the device (lg_cnn_load_from_trainer) and of the validation metrics
(lg_eval_logits, lg_cnn_evaluate; GraspPointSelector.load_from_trainer / evaluate, GraspTrainer.evaluate, fit(device_eval=True)).

The hand-off's contract is bit-identity with the host loader (lg_cnn_load on trainer.state_dict()): every buffer the kernels
read is compared with np.array_equal, and so are the logits.  Both entries run one fold (csrc/lg_cnn_load.hip: the host loader
stages its tensors on the device and runs what the hand-off runs), so their bit-identity follows from the shared path and
checks the staging and the two entries' plumbing; the bits themselves are pinned by an independent numpy float64 reference
(tests/cnn_fold_ref.py, proved in tests/test_cnn_fold_ref.py) in test_host_loader_equals_fold_reference.  The loader's
contract through the raw C-ABI (return codes, messages, what a refused load leaves) is test_loader_contract_through_the_c_abi.
The metrics' contract is the host twin (lg_eval_logits_host,
tests/test_eval_host.py checks that one against torch float64): equal counts, loss within 1e-12 * max(1, |ref|) -- the device's
and the host's exp / log1p differ in ulps only."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import synthetic_inputs as S  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402
from tests import cnn_fold_ref  # noqa: E402
from tests.test_eval_host import host_eval  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
# CASES of tests/test_train_oracle.py and ENCODERS of tests/test_gpu_train.py: padded channels (32 -> 64), four blocks, 512 filters,
# all four attention types
MODELS = [("spatial", (64, 128, 256)), ("spatial", (32, 64, 128)), ("channel", (32, 64, 128)), ("none", (128, 256, 512)),
          ("hybrid", (64, 128, 256)), ("hybrid", (64, 128, 256, 512))]
RTOL, ATOL = 1e-4, 1e-5   # the CNN path against float64 (tests/test_gpu_cnn_regimes.py)


def make_state(att, filt, seed=3):
    """Closed-form weights with seeded running statistics away from 0 / 1 (variances in [0.5, 2])."""
    p = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    rng = np.random.default_rng(1000 + seed + len(filt) * 7 + filt[0])
    for k in sorted(p):
        if k.endswith("running_mean"):
            p[k] = rng.uniform(-0.5, 0.5, p[k].shape).astype(np.float32)
        elif k.endswith("running_var"):
            p[k] = rng.uniform(0.5, 2.0, p[k].shape).astype(np.float32)
    return p


def make_trainer(att, filt, state=None, max_batch=16, **kw):
    from leafgrasp_amd.trainer import GraspTrainer
    tr = GraspTrainer(torch.device(DEV), attention_type=att, encoder_filters=filt, max_batch=max_batch, **kw)
    if state is not None:
        tr.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return tr


def selector():
    import leafgrasp_amd as L
    return L.GraspPointSelector(torch.device(DEV), load_model=False)


def all_buffers(sel):
    out = {}
    for which in ("bconv", "wconv", "uwino", "uwino4"):
        for layer in range(8):
            out[which, layer] = sel.cnn_weights(which, layer)
    for which in ("fcw", "fcb"):
        for layer in range(4):
            out[which, layer] = sel.cnn_weights(which, layer)
    for which in ("att_w", "ca_w1", "ca_b1", "ca_w2", "ca_b2", "zeros", "scalars"):
        out[which, 0] = sel.cnn_weights(which)
    return out


def assert_same_model(a, b, filt, att):
    """Every buffer of selector b (hand-off) equals selector a's (host loader), bit for bit; the expected ones exist."""
    ba, bb = all_buffers(a), all_buffers(b)
    n_layers = 2 * len(filt)
    for key in ba:
        assert ba[key].shape == bb[key].shape, key
        assert np.array_equal(ba[key].view(np.uint32), bb[key].view(np.uint32)), \
            (key, int((ba[key].view(np.uint32) != bb[key].view(np.uint32)).sum()), ba[key].size)
    standard = tuple(filt) == (64, 128, 256)
    for layer in range(8):
        on = layer < n_layers
        assert (bb["bconv", layer].size > 0) == on and (bb["uwino4", layer].size > 0) == on
        assert (bb["uwino", layer].size > 0) == (on and layer >= 1)
        assert (bb["wconv", layer].size > 0) == (on and (layer == 0 or standard))
    assert bb["uwino4", 0].size == 36 * 12 * ((filt[0] + 63) // 64 * 64)
    assert (bb["att_w", 0].size > 0) == (att in ("spatial", "hybrid")) and (bb["ca_w1", 0].size > 0) == (att in ("channel", "hybrid"))
    assert bb["zeros", 0].size == 4096 and not bb["zeros", 0].any()


def patches(n, seed):
    return torch.from_numpy(S.synthetic_patches(n, seed=seed)).to(DEV)


def assert_same_logits(a, b, state=None):
    for n, seed in ((5, 21), (37, 22)):
        x = patches(n, seed)
        la, lb = a.cnn_forward(x).cpu().numpy(), b.cnn_forward(x).cpu().numpy()
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (n, la, lb)
        if state is not None:
            ref = O.cnn_forward(state, x.cpu().numpy(), dtype=torch.float64)
            np.testing.assert_allclose(lb, ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("att,filt", MODELS)
def test_handoff_equals_host_loader(att, filt):
    state = make_state(att, filt)
    tr = make_trainer(att, filt, state)
    a, b = selector(), selector()
    a.set_cnn_state_dict(tr.state_dict())
    b.load_from_trainer(tr)
    assert b.ml_predictor is not None
    assert_same_model(a, b, filt, att)
    assert_same_logits(a, b, state)


@pytest.mark.parametrize("att,filt", MODELS)
def test_host_loader_equals_fold_reference(att, filt):
    """Every folded / transformed buffer lg_cnn_load leaves on the device equals the numpy float64 reference rounded once, bit
    for bit; the model has exactly the buffers the reference lists."""
    state = make_state(att, filt)
    ref = cnn_fold_ref.fold_reference(state)
    sel = selector()
    sel.set_cnn_state_dict(state)
    for which, layers in (("bconv", 8), ("wconv", 8), ("uwino", 8), ("uwino4", 8), ("fcw", 4), ("fcb", 4)):
        for layer in range(layers):
            got = sel.cnn_weights(which, layer)
            exp = ref.get((which, layer), np.empty(0, np.float32))
            assert got.shape == exp.shape, (which, layer, got.shape, exp.shape)
            diff = int((got.view(np.uint32) != exp.view(np.uint32)).sum())
            print(which, layer, got.size, "floats,", diff, "differ")
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (which, layer, diff, got.size)


def _hand_packed(filters, att_code, seed=2):
    """lg_cnn_weights of an encoder cnn.pack_state_dict refuses, filled field by field -> (struct, keepalive)."""
    from leafgrasp_amd._lib import LgCnnWeights
    att = {0: "spatial", 1: "channel", 2: "hybrid", 3: "none"}[att_code]
    state = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filters)
    keep = {k: np.ascontiguousarray(v, np.float32) for k, v in state.items()}
    ptr = lambda k: keep[k].ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    w = LgCnnWeights()
    w.n_blocks, w.attention_type, w.bn_eps = len(filters), att_code, 1e-5
    for b, f in enumerate(filters):
        w.filters[b] = f
        for j, (conv, bn) in enumerate(((0, 1), (3, 4))):
            L = 2 * b + j
            w.conv_w[L], w.conv_b[L] = ptr(f"encoder.{b}.{conv}.weight"), ptr(f"encoder.{b}.{conv}.bias")
            w.bn_g[L], w.bn_b[L] = ptr(f"encoder.{b}.{bn}.weight"), ptr(f"encoder.{b}.{bn}.bias")
            w.bn_m[L], w.bn_v[L] = ptr(f"encoder.{b}.{bn}.running_mean"), ptr(f"encoder.{b}.{bn}.running_var")
    assert att_code == 0, "spatial attention only"
    w.att_w, w.att_b = ptr("attention.0.weight"), ptr("attention.0.bias")
    for k, idx in enumerate((0, 4, 8, 12)):
        w.fc_w[k], w.fc_b[k] = ptr(f"classifier.{idx}.weight"), ptr(f"classifier.{idx}.bias")
        if k < 3:
            w.fbn_g[k], w.fbn_b[k] = ptr(f"classifier.{idx + 1}.weight"), ptr(f"classifier.{idx + 1}.bias")
            w.fbn_m[k], w.fbn_v[k] = ptr(f"classifier.{idx + 1}.running_mean"), ptr(f"classifier.{idx + 1}.running_var")
    return w, keep


def test_loader_contract_through_the_c_abi():
    """lg_cnn_load through the raw C-ABI: it starts from scratch (a refused load leaves no model), judges the geometry before
    the tensors and the attention type, and leaves a classifier size without a head kernel to the first forward."""
    from leafgrasp_amd._lib import LG_ERR_INVALID, LG_ERR_NO_MODEL, LG_ERR_UNSUPPORTED, LG_OK, lib
    from leafgrasp_amd.cnn import pack_state_dict
    sel = selector()
    h = sel._h
    x, logit = patches(1, 21), torch.zeros(1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    forward = lambda: lib.lg_cnn_forward(h, x.data_ptr(), 1, logit.data_ptr(), None)  # noqa: E731
    message = lambda: lib.lg_last_error(h).decode()  # noqa: E731
    state = make_state("spatial", (64, 128, 256))

    # 1. a refused load frees the model that was loaded
    w, keep = pack_state_dict(state)
    assert lib.lg_cnn_load(h, C.byref(w)) == LG_OK and forward() == LG_OK
    w.n_blocks = 5
    assert lib.lg_cnn_load(h, C.byref(w)) == LG_ERR_UNSUPPORTED
    assert forward() == LG_ERR_NO_MODEL
    # 2. a null encoder tensor
    w, keep = pack_state_dict(state)
    w.bn_g[3] = None
    assert lib.lg_cnn_load(h, C.byref(w)) == LG_ERR_INVALID
    assert "missing encoder tensor" in message()
    # 3. two blocks [32, 64]: the kernels take the encoder, lg_head_kernel has no instance for 64 filters on 8 x 8 pixels
    w, keep = _hand_packed((32, 64), 0)
    assert lib.lg_cnn_load(h, C.byref(w)) == LG_OK, message()
    assert forward() == LG_ERR_UNSUPPORTED
    assert "unsupported classifier size" in message()
    # 4. geometry is judged before the attention type
    w, keep = pack_state_dict(state)
    w.attention_type = 7
    w.filters[1] = 100
    assert lib.lg_cnn_load(h, C.byref(w)) == LG_ERR_UNSUPPORTED
    del keep


def test_refresh_in_place_after_a_training_step():
    """One optimisation step, then the hand-off again with no synchronisation in between: the call orders itself behind the
    trainer's stream, rewrites the buffers where they are (no allocation) and matches a fresh host load of the new state."""
    att, filt, n = "hybrid", (64, 128, 256), 8
    from leafgrasp_amd.trainer import dropout_layout
    tr = make_trainer(att, filt, make_state(att, filt))
    b = selector()
    b.load_from_trainer(tr)
    before = all_buffers(b)
    allocs = b.cnn_weights("allocs")
    assert allocs > 0
    x = b.cnn_forward(patches(37, 22))          # the activation workspace exists before the refresh
    x_dev, y_dev = patches(n, 11), torch.tensor([(i * 5 + 1) % 3 == 0 for i in range(n)], dtype=torch.float32, device=DEV)
    ones = [np.ones((n, w), np.float32) for w, _ in dropout_layout(filt)]
    mk = tr._masks_to_device(ones, n)
    logits = torch.empty(n, dtype=torch.float32, device=DEV)
    from leafgrasp_amd._lib import lib
    torch.cuda.current_stream().synchronize()
    # the asynchronous form of the step (no loss / norm read-back): it is still running when the hand-off is called
    rc = lib.lg_train_step(tr._h, x_dev.data_ptr(), y_dev.data_ptr(), n, mk.data_ptr(), tr.seed, C.byref(tr.hp), 1, None, None,
                           logits.data_ptr())
    assert rc == 0
    b.load_from_trainer(tr)
    assert b.cnn_weights("allocs") == allocs, "an in-place refresh allocates nothing: the buffers sit where they sat"
    tr.num_batches_tracked += 1
    a = selector()
    a.set_cnn_state_dict(tr.state_dict())
    assert_same_model(a, b, filt, att)
    assert_same_logits(a, b)
    after = all_buffers(b)
    assert not np.array_equal(before["uwino4", 3], after["uwino4", 3]), "the step moved the weights"
    assert not np.array_equal(x.cpu().numpy(), b.cnn_forward(patches(37, 22)).cpu().numpy())


def test_geometry_change_and_refusal():
    from leafgrasp_amd._lib import LG_ERR_INVALID, LG_ERR_UNSUPPORTED, LgError
    b = selector()
    for att, filt in (("spatial", (64, 128, 256)), ("hybrid", (64, 128, 256, 512))):
        state = make_state(att, filt, seed=5)
        tr = make_trainer(att, filt, state)
        a = selector()
        a.set_cnn_state_dict(tr.state_dict())
        b.load_from_trainer(tr)
        assert_same_model(a, b, filt, att)
        assert_same_logits(a, b, state)
    x = patches(5, 21)
    kept = b.cnn_forward(x).cpu().numpy()
    kept_buffers = all_buffers(b)
    # the trainer takes two blocks; the inference kernels do not
    small = make_trainer("spatial", (32, 64))
    with pytest.raises(LgError, match=f"status {LG_ERR_UNSUPPORTED}:"):
        b.load_from_trainer(small)
    assert np.array_equal(kept, b.cnn_forward(x).cpu().numpy())
    now = all_buffers(b)
    assert all(np.array_equal(kept_buffers[k], now[k]) for k in now)

    class Gone:   # a trainer whose handle has been destroyed
        _h = C.c_void_p()
    for dead in (Gone(), object()):
        with pytest.raises(LgError, match=f"status {LG_ERR_INVALID}:"):
            b.load_from_trainer(dead)
    small.__del__()
    assert not small._h
    with pytest.raises(LgError, match=f"status {LG_ERR_INVALID}:"):
        b.load_from_trainer(small)
    assert np.array_equal(kept, b.cnn_forward(x).cpu().numpy())


def _metric_sets():
    g = np.load(os.path.join(HERE, "golden", "train_host_vectors.npz"))
    rng = np.random.default_rng(37)
    return [(g["ap_outputs"].reshape(-1), g["ap_labels"], 16, 2.0, 0.5),
            ((rng.standard_normal(37) * 3).astype(np.float32), (rng.random(37) < 0.4).astype(np.float32), 16, 2.0, 0.5),
            ((rng.standard_normal(37) * 3).astype(np.float32), (rng.random(37) < 0.4).astype(np.float32), 5, 3.5, -0.25)]


def test_metrics_on_the_device_equal_the_host_twin():
    sel = selector()
    for z, y, chunk, pw, thr in _metric_sets():
        ref = host_eval(z, y, chunk, pw, thr)
        zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
        r1 = sel.eval_logits(zt, yt, batch_size=chunk, pos_weight=pw, threshold=thr)
        r2 = sel.eval_logits(zt, yt, batch_size=chunk, pos_weight=pw, threshold=thr)
        for f in ("n", "n_chunks", "correct", "tp", "fp", "fn", "tn"):
            assert getattr(r1, f) == getattr(ref, f) == getattr(r2, f), f
        print("loss device", repr(r1.loss), "host", repr(ref.loss))
        assert abs(r1.loss - ref.loss) <= 1e-12 * max(1.0, abs(ref.loss))
        assert np.float64(r1.loss).view(np.uint64) == np.float64(r2.loss).view(np.uint64)
    z, y = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    from leafgrasp_amd._lib import LG_ERR_INVALID, LgError
    with pytest.raises(LgError, match=f"status {LG_ERR_INVALID}:"):
        sel.eval_logits(z, y, batch_size=0)
    nan = torch.tensor([1.0, float("nan"), -2.0, 0.7], device=DEV)
    r = sel.eval_logits(nan, torch.tensor([1.0, 1.0, 0.0, 0.0], device=DEV), batch_size=2)
    assert np.isnan(r.loss) and (r.tp, r.fp, r.fn, r.tn, r.correct) == (1, 1, 1, 1, 2)


def test_evaluate_end_to_end():
    att, filt, n = "spatial", (64, 128, 256), 37
    tr = make_trainer(att, filt, make_state(att, filt), pos_weight=2.0)
    x = patches(n, 23)
    y = torch.from_numpy((np.random.default_rng(5).random(n) < 0.4).astype(np.float32)).to(DEV)
    sel = selector()
    ev = tr.evaluate(x, y, selector=sel, batch_size=16, return_logits=True)
    assert set(ev) == {"val_loss", "accuracy", "n", "metrics", "logits"} and ev["n"] == n
    assert set(tr.evaluate(x, y, selector=sel)) == {"val_loss", "accuracy", "n", "metrics"}
    logits = tr.predict_logits(x)                      # the host route: state_dict + lg_cnn_load + lg_cnn_forward
    got = ev["logits"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), logits.cpu().numpy().view(np.uint32))
    assert tr.evaluate(x, y, selector=sel)["val_loss"] == ev["val_loss"]     # without logits_out: the same number
    ref = host_eval(got, y.cpu().numpy(), 16, 2.0, 0.5)
    from leafgrasp_amd.trainer import analyze_predictions, metrics_from_counts
    assert ev["metrics"] == metrics_from_counts(ref.tp, ref.fp, ref.fn, ref.tn) == analyze_predictions(logits, y)
    assert ev["accuracy"] == 100.0 * ref.correct / n
    assert ref.correct == int(((torch.sigmoid(logits) > 0.5).float() == y).sum().item())
    assert abs(ev["val_loss"] - ref.loss) <= 1e-12 * max(1.0, abs(ref.loss))
    # fit()'s present float32 loop on the same logits: fp32 eps ~6e-8 over sums of 16 gives ~1e-6; a factor of ten of margin
    # because torch's reduction order is not ours
    vb = [tr.bce_with_logits(logits[s:s + 16], y[s:s + 16]).item() for s in range(0, n, 16)]
    loop = float(np.mean(vb))
    print("val_loss device", repr(ev["val_loss"]), "float32 loop", repr(loop))
    assert abs(ev["val_loss"] - loop) <= 1e-5 * abs(loop)


def test_fit_with_device_eval_matches_the_host_route(tmp_path):
    rng = np.random.default_rng(0)
    n = 64
    x = S.synthetic_patches(n, seed=40)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x[y == 1, 2] += 0.8
    hist = {}
    for dev_eval in (False, True):
        tr = make_trainer("spatial", (64, 128, 256), seed=7)
        d = tmp_path / ("dev" if dev_eval else "host")
        hist[dev_eval] = tr.fit(x, y, num_epochs=2, batch_size=16, save_dir=str(d), log=None, device_eval=dev_eval)
    h, g = hist[False], hist[True]
    assert len(g["val_losses"]) == 2
    assert g["metrics_history"] == h["metrics_history"]
    print("val_losses host", h["val_losses"], "device", g["val_losses"])
    for a, b in zip(h["val_losses"], g["val_losses"]):
        assert abs(a - b) <= 1e-5 * abs(a)
    # validation does not touch training: the same steps, the same bits
    assert [np.float64(v).view(np.uint64) for v in g["train_losses"]] == [np.float64(v).view(np.uint64) for v in h["train_losses"]]
    sel = selector()
    sel.load_ml_model(str(tmp_path / "dev" / "best_model.pth"))
    assert sel.ml_predictor is not None
    ck = torch.load(tmp_path / "dev" / "best_model.pth", map_location="cpu", weights_only=True)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "metrics", "train_losses", "val_losses",
            "metrics_history", "normalization_stats"} == set(ck)
