"""GPU parity of the training step (lg_train_step through the C-ABI) against the reference fixture
(tests/golden/train_vectors.npz: reference module + torch.optim.Adam) and against the oracle's restated step on the same
seeded inputs with explicit dropout masks.  Floating point: fp32 sums in a different order than torch's; tolerances are
written at each comparison.  A training step is not continuous in its inputs (ReLU / max-pool decisions), see
tests/test_train_oracle.py::assert_close_robust."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import synthetic_inputs as S  # noqa: E402
from oracle import lg_oracle as O  # noqa: E402
from tests.test_train_oracle import CASES, assert_close_robust, case_inputs, noisy_bias  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def make_trainer(att, filt, max_batch, **kw):
    from leafgrasp_amd.trainer import GraspTrainer
    return GraspTrainer(torch.device(DEV), attention_type=att, encoder_filters=filt, max_batch=max_batch, **kw)


def ones_masks(filt, n):
    from leafgrasp_amd.trainer import dropout_layout
    return [np.ones((n, w), np.float32) for w, _ in dropout_layout(filt)]


def random_masks(filt, n, seed):
    from leafgrasp_amd.trainer import dropout_layout
    rng = np.random.default_rng(seed)
    return [((rng.random((n, w)) >= p) / (1.0 - p)).astype(np.float32) for w, p in dropout_layout(filt)]


def compare_step(tr, ref, loss, logits, gnorm, tight=True):
    """tr: trainer after the step; ref: oracle result dict of the same step."""
    assert loss == pytest.approx(ref["loss"], rel=2e-5 if tight else 2e-3)
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"], rtol=1e-4 if tight else 1e-2, atol=2e-5 if tight else 2e-3)
    assert gnorm == pytest.approx(ref["grad_norm"], rel=2e-4 if tight else 2e-2)
    g = tr.gradients()
    errs = {}
    for k, gr in ref["grads"].items():
        den = float(np.linalg.norm(gr))
        if den < 1e-4 * ref["grad_norm"] / np.sqrt(len(ref["grads"])):
            # biases in front of a BatchNorm: mathematically zero gradient (torch: rounding noise, here: exact zero / noise)
            assert float(np.abs(g[k].numpy()).max()) <= 1e-4 * max(1.0, ref["grad_norm"]), k
            continue
        errs[k] = float(np.linalg.norm(g[k].numpy() - gr)) / den
    # One activation within rounding of a ReLU / max-pool decision, decided differently by the two implementations, moves
    # the gradient of its BatchNorm channel and of every layer below it by ~0.3 % (measured: tests/tools/train_diag.py,
    # where torch fp32 and this path sit equally close to torch fp64 on every tensor above the flip).  Hence: every tensor
    # within 2 % in relative L2 (a wrong kernel is off by >= 10 %), the classifier tensors (few decisions, far above the
    # encoder's) within 2e-4.
    for k, e in errs.items():
        assert e <= (2e-2 if tight else 8e-2), (k, e, errs)
        if k.startswith("classifier") and tight:
            assert e <= 2e-4, (k, e)


def assert_adam_replay(tr, sd, params, names, own_g, own_norm):
    """clip_grad_norm_ + torch.optim.Adam replayed on the host in float32 from the trainer's own gradients (own_g, own_norm:
    one entry per step from `params`) must give the trainer's parameters `sd` to rounding, every element of every tensor."""
    hp = tr.hp
    lr, b1, b2, eps_, wd, mx = (np.float32(v) for v in (hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.max_grad_norm))
    one = np.float32(1.0)
    for k in names:
        pk = np.asarray(params[k], np.float32).copy()
        m = np.zeros_like(pk)
        v = np.zeros_like(pk)
        for t_, (gd, gn) in enumerate(zip(own_g, own_norm), start=1):
            coef = min(mx / (np.float32(gn) + np.float32(1e-6)), one)
            gi = gd[k].astype(np.float32) * coef + wd * pk
            m = b1 * m + (one - b1) * gi
            v = b2 * v + (one - b2) * gi * gi
            bc1, bc2 = one - b1 ** np.float32(t_), one - b2 ** np.float32(t_)
            pk = pk - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps_))
        # (fp32 rounding of g * coef + wd * p where the two terms nearly cancel is amplified by 1 / sqrt(v): up to ~1e-6, 0.2 % of lr)
        np.testing.assert_allclose(sd[k].numpy(), pk, rtol=2e-6, atol=2.5e-6, err_msg=f"Adam replay {k}")


@pytest.mark.parametrize("att,filt,n", CASES)
def test_train_step_matches_reference_fixture(att, filt, n):
    """Step 0 from the closed-form weights: loss, logits, total and per-tensor gradient norms, sampled gradients, BatchNorm
    running statistics, Adam moments and updated parameters against the reference module + torch.optim.Adam."""
    tv = np.load(os.path.join(HERE, "golden", "train_vectors.npz"))
    tag = f"{att}_{len(filt)}x{filt[0]}"
    params, x, y = case_inputs(att, filt, n)
    names = [str(k) for k in tv[f"{tag}_names"]]
    pick = tv[f"{tag}_pick"]
    tr = make_trainer(att, filt, 16)
    from leafgrasp_amd.trainer import parameter_layout
    assert [k for k, _ in parameter_layout(filt, att)[0]] == names     # model.named_parameters() order of the reference
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    loss, logits, gnorm = tr.train_step(x, y, masks=ones_masks(filt, n), return_logits=True)
    own_g = [{k: v.numpy().copy() for k, v in tr.gradients().items()}]   # this path's own gradients, step by step
    own_norm = [gnorm]
    assert loss == pytest.approx(float(tv[f"{tag}_loss0"]), rel=2e-5)
    np.testing.assert_allclose(logits.cpu().numpy(), tv[f"{tag}_logits0"], rtol=1e-4, atol=2e-5)
    assert gnorm == pytest.approx(float(tv[f"{tag}_gnorm0"]), rel=2e-4)
    g = tr.gradients()
    gt = np.array([np.linalg.norm(g[k].numpy().astype(np.float64)) for k in names])
    # flip-tolerant bounds (see compare_step): a decision flip moves the tensors below it by ~0.3 %
    assert_close_robust(gt, tv[f"{tag}_gtnorm0"], 1e-2, 1e-5, 0.0, what="per-tensor gradient norms")
    gs = np.stack([g[k].numpy().reshape(-1)[pick[i]] for i, k in enumerate(names)])
    ref_gs = tv[f"{tag}_gsample0"]
    for i, k in enumerate(names):   # relative L2 over the 48 sampled entries of every tensor with a real gradient
        if np.linalg.norm(ref_gs[i]) > 1e-4 * float(tv[f"{tag}_gnorm0"]) / np.sqrt(len(names)):
            assert np.linalg.norm(gs[i] - ref_gs[i]) <= 3e-2 * np.linalg.norm(ref_gs[i]), k
    tight = np.array([k.startswith("classifier") and not noisy_bias(k) for k in names])
    assert_close_robust(gs[tight], tv[f"{tag}_gsample0"][tight], 1e-3, 2e-5, 0.01, 2e-4, what="classifier gradient samples")
    # second step: Adam state carried on the device
    loss1, logits1, gnorm1 = tr.train_step(x, y, masks=ones_masks(filt, n), return_logits=True)
    own_g.append({k: v.numpy().copy() for k, v in tr.gradients().items()})
    own_norm.append(gnorm1)
    assert loss1 == pytest.approx(float(tv[f"{tag}_loss1"]), rel=2e-3)
    assert gnorm1 == pytest.approx(float(tv[f"{tag}_gnorm1"]), rel=3e-2)
    np.testing.assert_allclose(logits1.cpu().numpy(), tv[f"{tag}_logits1"], rtol=1e-2, atol=5e-3)
    sd, opt = tr.state_dict(), tr.optimizer_state()
    assert opt["step"] == 2 and int(sd["encoder.0.1.num_batches_tracked"]) == int(tv[f"{tag}_nbt"])
    buf = np.concatenate([sd[k].numpy().reshape(-1) for k in sd if "running_" in k])
    # after two steps: the second forward ran on parameters that took one Adam step (noise-sign steps where the gradient
    # is rounding noise); one-step running statistics are checked tightly in the oracle comparison below
    np.testing.assert_allclose(buf, tv[f"{tag}_buffers"], rtol=2e-3, atol=1e-3)
    ms = np.stack([opt["exp_avg"][k].numpy().reshape(-1)[pick[i]] for i, k in enumerate(names)])
    vs = np.stack([opt["exp_avg_sq"][k].numpy().reshape(-1)[pick[i]] for i, k in enumerate(names)])
    ps = np.stack([sd[k].numpy().reshape(-1)[pick[i]] for i, k in enumerate(names)])
    # second-step moments: the step-2 gradient already differs by flips and by the noise-sign parameter steps of step 1
    # (torch fp32 vs fp64 differ the same way, tests/test_train_oracle.py); a wrong beta / bias correction is off by 2x
    assert np.linalg.norm(ms - tv[f"{tag}_msample"]) <= 0.05 * np.linalg.norm(tv[f"{tag}_msample"])
    assert np.linalg.norm(vs - tv[f"{tag}_vsample"]) <= 0.10 * np.linalg.norm(tv[f"{tag}_vsample"])
    noisy = np.array([noisy_bias(k) for k in names])
    # Parameters after two optimisation steps.
    # (1) The optimiser itself, free of any ReLU / max-pool decision: clip_grad_norm_(1.0) + torch.optim.Adam (L2 weight decay,
    #     bias corrections; scripts/train_model.py:247-265) replayed on the host in float32 from THIS path's own two gradients
    #     must give this path's parameters to rounding, every element of every tensor.
    assert_adam_replay(tr, sd, params, names, own_g, own_norm)
    # (2) Against the reference fixture.  Adam's first update is lr * sign(g) and later ones depend on RATIOS of gradients, so a
    #     parameter can only leave the fixture's value where this path's gradient element differs from the reference's: where the
    #     sampled gradients of BOTH steps agree (every tensor within 1e-3 of its RMS: no ReLU / max-pool decision fell the other
    #     way in this case) at most 1 % of the elements may miss 1e-4; where a decision did flip (the fixture's second step of the
    #     'hybrid' case and both steps of the 'channel' case do: gradients of whole tensors move by up to 1.7 % of their RMS) the
    #     parameters are only held to the optimiser's own bound of 2 * lr per step -- (1) above is the check that cannot be
    #     fooled there.
    ref_p = tv[f"{tag}_psample"]
    agree = True
    for step in range(2):
        ref_g = tv[f"{tag}_gsample{step}"]
        rms = np.sqrt((ref_g.astype(np.float64) ** 2).mean(axis=1, keepdims=True)) + 1e-30
        own = np.stack([own_g[step][k].reshape(-1)[pick[i]] for i, k in enumerate(names)])
        agree &= bool((np.abs(own - ref_g) / rms)[~noisy].max() <= 1e-3)
    bad = np.abs(ps - ref_p) > 2e-5 + 1e-4 * np.abs(ref_p)
    if agree:
        assert bad[~noisy].mean() <= 0.01, float(bad[~noisy].mean())
    np.testing.assert_allclose(ps, ref_p, atol=2 * 2 * 0.0005 + 1e-6)


@pytest.mark.parametrize("att,filt,n,seed", [("spatial", (64, 128, 256), 16, 1), ("none", (64, 128, 256, 512), 8, 2),
                                             ("spatial", (128, 256, 512), 5, 3), ("spatial", (32, 64, 128), 16, 4),
                                             ("spatial", (64, 128, 256), 128, 5), ("channel", (64, 128, 256), 16, 6),
                                             ("hybrid", (64, 128, 256, 512), 8, 7)])
def test_train_step_with_dropout_masks_vs_oracle(att, filt, n, seed):
    """The reference's batch size (16) and every encoder_filters configuration of its sweep, plus a batch of 128 (the
    large-tile convolution shape, BatchNorm reductions split over sample chunks), with random Dropout2d /
    Dropout keep masks handed to both sides; first step from the closed-form weights and a second step from the ORACLE's
    state after the first (parameters, running statistics, Adam moments, step count loaded into the trainer)."""
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=20 + seed)
    y = (np.random.default_rng(seed).random(n) < 0.4).astype(np.float32)
    y[0], y[1] = 0.0, 1.0
    tr = make_trainer(att, filt, max(16, n))
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    mk = random_masks(filt, n, seed)
    ref = O.cnn_train_step(params, x, y, masks=mk)
    loss, logits, gnorm = tr.train_step(x, y, masks=mk, return_logits=True)
    compare_step(tr, ref, loss, logits, gnorm)
    sd = tr.state_dict()
    for k in ref["params"]:
        if "running_" in k:
            np.testing.assert_allclose(sd[k].numpy(), ref["params"][k], rtol=1e-4, atol=1e-5, err_msg=k)
    # second step from the oracle's state
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in ref["params"].items()},
                       {"exp_avg": ref["opt_state"]["exp_avg"], "exp_avg_sq": ref["opt_state"]["exp_avg_sq"], "step": 1})
    mk2 = random_masks(filt, n, seed + 100)
    ref2 = O.cnn_train_step(ref["params"], x, y, masks=mk2, opt_state=ref["opt_state"])
    loss2, logits2, gnorm2 = tr.train_step(x, y, masks=mk2, return_logits=True)
    compare_step(tr, ref2, loss2, logits2, gnorm2, tight=False)
    opt = tr.optimizer_state()
    assert opt["step"] == 2
    for k in ref2["opt_state"]["exp_avg"]:
        assert_close_robust(opt["exp_avg"][k].numpy(), ref2["opt_state"]["exp_avg"][k], 2e-2, 1e-5, 0.05, 0.08, what="m " + k)
        assert_close_robust(opt["exp_avg_sq"][k].numpy(), ref2["opt_state"]["exp_avg_sq"][k], 4e-2, 1e-9, 0.05, 0.1, what="v " + k)


# lgt_conv_kernel's three shapes (lgt_conv in lg_train_conv.hip; forward and dgrad): large (256 px x 64 channels, several samples
# per tile on the 8 x 8 and 4 x 4 layers), small, K-split.  The thresholds are read at lg_train_create: the environment forces
# one form on every layer it can take (the K-split needs 32 input channels; layer 0 keeps its own choice there).
CONV_FORMS = {"large": {"LG_TRAIN_CONV_SMALL": "0", "LG_TRAIN_CONV_SPLIT": "0"},
              "small": {"LG_TRAIN_CONV_SMALL": "1073741824", "LG_TRAIN_CONV_SPLIT": "0"},
              "split": {"LG_TRAIN_CONV_SPLIT": "1073741824"}}
ENCODERS = [("spatial", (64, 128, 256)), ("spatial", (32, 64, 128)), ("none", (128, 256, 512)), ("hybrid", (64, 128, 256, 512))]


def _first_step_vs_oracle(tr, params, x, y, filt, seed):
    mk = random_masks(filt, len(x), seed)
    ref = O.cnn_train_step(params, x, y, masks=mk)
    loss, logits, gnorm = tr.train_step(x, y, masks=mk, return_logits=True)
    compare_step(tr, ref, loss, logits, gnorm, tight=True)
    sd = tr.state_dict()
    for k in ref["params"]:
        if "running_" in k:
            np.testing.assert_allclose(sd[k].numpy(), ref["params"][k], rtol=1e-4, atol=1e-5, err_msg=k)
    return gnorm


@pytest.mark.parametrize("form", list(CONV_FORMS))
@pytest.mark.parametrize("att,filt", ENCODERS, ids=["standard", "lightweight", "wide", "deep"])
def test_train_step_every_conv_form_on_ragged_tiles(monkeypatch, att, filt, form):
    """13 samples: ragged against every multi-sample tile of the large form (4 samples at 8 x 8, 16 at 4 x 4)."""
    n, seed = 13, 40
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=seed)
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    for k, v in CONV_FORMS[form].items():
        monkeypatch.setenv(k, v)
    tr = make_trainer(att, filt, 16)
    for k in CONV_FORMS[form]:
        monkeypatch.delenv(k)
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    _first_step_vs_oracle(tr, params, x, y, filt, seed)


def test_train_step_at_the_natural_large_form_batch():
    """258 samples with the default thresholds: the 8 x 8 layers take the large form with a half-filled last tile and the
    BatchNorm reductions run in sample chunks.  Step one against the oracle; two steps against the host replay of Adam."""
    att, filt, n, seed = "spatial", (64, 128, 256), 258, 41
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=seed)
    y = (np.random.default_rng(seed).random(n) < 0.4).astype(np.float32)
    tr = make_trainer(att, filt, n)
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    own_norm = [_first_step_vs_oracle(tr, params, x, y, filt, seed)]
    own_g = [{k: v.numpy().copy() for k, v in tr.gradients().items()}]
    _, _, gnorm1 = tr.train_step(x, y, masks=random_masks(filt, n, seed + 100), return_logits=True)
    own_g.append({k: v.numpy().copy() for k, v in tr.gradients().items()})
    own_norm.append(gnorm1)
    from leafgrasp_amd.trainer import parameter_layout
    names = [k for k, _ in parameter_layout(filt, att)[0]]
    assert tr.optimizer_state()["step"] == 2
    assert_adam_replay(tr, tr.state_dict(), params, names, own_g, own_norm)


def test_gradients_only_and_determinism():
    """apply_update=False leaves parameters and optimizer untouched; two identical steps give identical bits (every
    reduction of the path is ordered)."""
    att, filt, n = "spatial", (64, 128, 256), 16
    params = S.cnn_closed_form_params(seed=5, attention_type=att, filters=filt)
    x, y = S.synthetic_patches(n, seed=31), (np.arange(n) % 3 == 0).astype(np.float32)
    mk = random_masks(filt, n, 9)
    out = []
    for _ in range(2):
        tr = make_trainer(att, filt, 16)
        tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        l0 = tr.train_step(x, y, masks=mk, apply_update=False)
        sd0 = tr.state_dict()
        for k, v in params.items():
            if "running_" not in k:
                np.testing.assert_array_equal(sd0[k].numpy(), v)
        assert tr.optimizer_state()["step"] == 0
        l1 = tr.train_step(x, y, masks=mk)
        out.append((l0, l1, tr._get(params=True, grads=True, m=True, v=True)))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    for key in ("params", "grads", "exp_avg", "exp_avg_sq"):
        np.testing.assert_array_equal(out[0][2][key], out[1][2][key])


def test_training_reduces_loss_and_feeds_inference_path(tmp_path):
    """A short run on a separable synthetic set with device-drawn dropout masks: the loss falls, the eval-mode logits of
    the trained weights (running statistics, lg_cnn_forward) agree with the oracle's eval forward on the same state dict,
    and fit() writes a checkpoint that GraspPointSelector.load_ml_model reads."""
    import leafgrasp_amd as L
    rng = np.random.default_rng(0)
    n = 96
    x = S.synthetic_patches(n, seed=40)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x[y == 1, 2] += 0.8          # positives: brighter third channel
    tr = make_trainer("spatial", (64, 128, 256), 16, seed=7)
    yt = torch.from_numpy(y).to(DEV)
    eval_before = float(tr.bce_with_logits(tr.predict_logits(x), yt))
    first, last = [], []
    for epoch in range(12):
        perm = rng.permutation(n)
        for s in range(0, n, 16):
            b = perm[s:s + 16]
            loss = tr.train_step(x[b], y[b])
            (first if epoch == 0 else last if epoch == 11 else []).append(loss)
    assert np.mean(last) < 0.6 * np.mean(first), (np.mean(first), np.mean(last))
    sd = tr.state_dict()
    logits = tr.predict_logits(x[:32]).cpu().numpy()
    # TRAINED weights (BN statistics and scales as 70 Adam steps left them) through the inference path -- Winograd F(4x4,3x3)
    # -- against the float64 oracle at the path's 1e-4 bar (atol: 1e-4 of the largest logit, for logits near zero)
    ref = O.cnn_forward({k: v.numpy() for k, v in sd.items() if not k.endswith("num_batches_tracked")}, x[:32], dtype=torch.float64)
    np.testing.assert_allclose(logits, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref).max()))
    eval_after = float(tr.bce_with_logits(tr.predict_logits(x), yt))     # model.eval(): running statistics, no dropout
    assert eval_after < eval_before, (eval_before, eval_after)
    hist = tr.fit(x, y, num_epochs=2, batch_size=16, save_dir=str(tmp_path), log=None)
    assert len(hist["val_losses"]) == 2 and os.path.exists(tmp_path / "best_model.pth")
    sel = L.GraspPointSelector(torch.device(DEV), load_model=False)
    sel.load_ml_model(str(tmp_path / "best_model.pth"))
    assert sel.ml_predictor is not None
    ck = torch.load(tmp_path / "best_model.pth", map_location="cpu", weights_only=True)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "metrics", "train_losses", "val_losses"} <= set(ck)
    # the optimizer state is in torch.optim.Adam's own layout: a stock Adam over same-shaped parameters loads it, and the
    # trainer resumes from it bit for bit
    from leafgrasp_amd.trainer import parameter_layout
    plist = [torch.nn.Parameter(torch.zeros(shape)) for _, shape in parameter_layout((64, 128, 256), "spatial")[0]]
    topt = torch.optim.Adam(plist, lr=0.1)
    topt.load_state_dict(ck["optimizer_state_dict"])
    assert topt.param_groups[0]["lr"] == pytest.approx(0.0005) and topt.param_groups[0]["weight_decay"] == pytest.approx(0.01)
    osd = tr.torch_optimizer_state_dict()
    assert int(osd["state"][0]["step"]) == tr.optimizer_state()["step"] > 0
    tr2 = make_trainer("spatial", (64, 128, 256), 16, seed=7)
    tr2.load_torch_optimizer_state_dict(osd, tr.state_dict())
    a, b = tr._get(params=True, m=True, v=True), tr2._get(params=True, m=True, v=True)
    for key in ("params", "exp_avg", "exp_avg_sq"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["step"] == b["step"]


def test_rejects_bad_arguments():
    from leafgrasp_amd.trainer import GraspTrainer
    with pytest.raises(ValueError):
        GraspTrainer(torch.device(DEV), attention_type="cbam")
    tr = make_trainer("spatial", (64, 128, 256), 8)
    with pytest.raises(ValueError):
        tr.train_step(np.zeros((1, 9, 32, 32), np.float32), np.zeros(1, np.float32))     # BatchNorm needs N > 1
    with pytest.raises(ValueError):
        tr.train_step(np.zeros((9, 9, 32, 32), np.float32), np.zeros(9, np.float32))     # > max_batch
    with pytest.raises(ValueError):
        tr.train_step(np.zeros((4, 9, 32, 32), np.float32), np.zeros(4, np.float32), masks=[np.ones((4, 64), np.float32)])


_DDP_WORKER = r"""
import os, sys
sys.path.insert(0, %(repo)r)
import numpy as np, torch, torch.distributed as dist
import synthetic_inputs as S
from leafgrasp_amd.trainer import GraspTrainer, dropout_layout
dist.init_process_group("gloo")            # two ranks on ONE device here; on a node: backend 'nccl' (= RCCL), one GPU per rank
rank, world = dist.get_rank(), dist.get_world_size()
filt = (64, 128, 256)
params = S.cnn_closed_form_params(seed=8, attention_type="spatial", filters=filt)
x = S.synthetic_patches(16, seed=50)
y = (np.arange(16) %% 3 == 0).astype(np.float32)
sl = slice(rank * 8, rank * 8 + 8)
rng = np.random.default_rng(70 + rank)
masks = [((rng.random((8, w)) >= p) / (1.0 - p)).astype(np.float32) for w, p in dropout_layout(filt)]
tr = GraspTrainer(torch.device("cuda:0"), encoder_filters=filt, max_batch=8)
tr.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
loss = tr.train_step_ddp(x[sl], y[sl], dist, masks=masks)
out = tr._get(params=True, grads=True, m=True, v=True)
np.savez(os.path.join(%(out)r, f"rank{rank}.npz"), loss=loss, step=out["step"], **{k: v for k, v in out.items() if k != "step"})
dist.barrier()
dist.destroy_process_group()
"""


def test_data_parallel_step_two_ranks(tmp_path):
    """Two processes (gloo, both on this one GPU -- the multi-GPU launch uses 'nccl' = RCCL with a GPU per rank): each runs
    forward + backward on its half of a 16-sample batch, the flat gradient vectors are averaged with one all-reduce, both
    apply clip + Adam.  The ranks end with identical parameters; the averaged gradient and the update equal the oracle's
    (two restated half-batch steps averaged, then the restated clip + Adam)."""
    import socket
    import subprocess
    import sys
    from leafgrasp_amd.trainer import dropout_layout, parameter_layout
    script = tmp_path / "ddp_worker.py"
    script.write_text(_DDP_WORKER % {"repo": os.path.dirname(HERE), "out": str(tmp_path)})
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), str(script)], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["step"]) == 1 and int(r1["step"]) == 1
    for k in ("params", "grads", "exp_avg", "exp_avg_sq"):      # same averaged gradient -> same update, bit for bit
        np.testing.assert_array_equal(r0[k], r1[k])
    filt = (64, 128, 256)
    params = S.cnn_closed_form_params(seed=8, attention_type="spatial", filters=filt)
    x = S.synthetic_patches(16, seed=50)
    y = (np.arange(16) % 3 == 0).astype(np.float32)
    refs = []
    for rank in range(2):
        rng = np.random.default_rng(70 + rank)
        masks = [((rng.random((8, w)) >= p) / (1.0 - p)).astype(np.float32) for w, p in dropout_layout(filt)]
        refs.append(O.cnn_train_step(params, x[rank * 8:rank * 8 + 8], y[rank * 8:rank * 8 + 8], masks=masks, apply_update=False))
    assert float(r0["loss"]) == pytest.approx(refs[0]["loss"], rel=2e-5) and float(r1["loss"]) == pytest.approx(refs[1]["loss"], rel=2e-5)
    names = [k for k, _ in parameter_layout(filt, "spatial")[0]]
    gavg = np.concatenate([(0.5 * (refs[0]["grads"][k] + refs[1]["grads"][k])).reshape(-1) for k in names])
    assert np.linalg.norm(r0["grads"] - gavg) <= 2e-2 * np.linalg.norm(gavg)
    # restated clip + first Adam step on the averaged gradient (train_model.py:256-258)
    p0 = np.concatenate([params[k].reshape(-1) for k in names]).astype(np.float64)
    g = r0["grads"].astype(np.float64)          # the update is checked on the gradient the ranks actually shared
    coef = min(1.0 / (np.linalg.norm(g) + 1e-6), 1.0)
    g = g * coef + 0.01 * p0
    m, v = 0.1 * g, 0.001 * g * g
    expect = p0 - (0.0005 / 0.1) * (m / (np.sqrt(v) / np.sqrt(0.001) + 1e-8))
    np.testing.assert_allclose(r0["exp_avg"], m, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(r0["params"], expect, rtol=1e-5, atol=2e-6)


def test_train_grasp_model_entry_point(tmp_path):
    """scripts/train_model.py::train_grasp_model on a small training_data.pt in the data collector's layout: the file is
    read (weights_only), features prepared, two epochs run, best_model.pth / final_model.pth written with the reference's
    checkpoint keys and readable by GraspPointSelector.load_ml_model."""
    import leafgrasp_amd as L
    from leafgrasp_amd.trainer import train_grasp_model
    rng = np.random.default_rng(5)
    n = 80
    labels = (rng.random(n) < 0.45).astype(np.int64)
    scores = rng.random((n, 7, 32, 32)).astype(np.float32)
    scores[labels == 1, 0] += 0.5
    data = {"depth_patches": torch.from_numpy(rng.random((n, 32, 32)).astype(np.float32) * 0.3 + 0.3),
            "mask_patches": torch.from_numpy((rng.random((n, 32, 32)) > 0.3).astype(np.float32)),
            "score_patches": torch.from_numpy(scores), "labels": torch.from_numpy(labels)}
    torch.save(data, tmp_path / "training_data.pt")
    hist = train_grasp_model(str(tmp_path / "training_data.pt"), str(tmp_path / "models"), device=DEV, num_epochs=2, log=None)
    assert len(hist["train_losses"]) == 2 and np.isfinite(hist["best_val_loss"])
    for name in ("best_model.pth", "final_model.pth"):
        ck = torch.load(tmp_path / "models" / name, map_location="cpu", weights_only=True)
        assert {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "metrics", "normalization_stats",
                "train_losses", "val_losses", "metrics_history"} <= set(ck)
        assert set(ck["normalization_stats"]) == {"depth_mean", "depth_std", "score_mean", "score_std"}
    sel = L.GraspPointSelector(torch.device(DEV), load_model=False)
    sel.load_ml_model(str(tmp_path / "models" / "best_model.pth"))
    assert sel.ml_predictor is not None
