"""The train-mode forward of oracle.lg_oracle.cnn_train_step restated so that its DECISIONS are visible (CPU, torch).

A training step is smooth except where a ReLU or a 2 x 2 max-pool decides: a pre-activation within rounding of zero, or two
pool entries within rounding of each other, decided the other way, moves every tensor below by ~0.3 %.  step() returns, for
every ReLU, the pre-activation ("z"), and for every pool cell whose maximum is positive the gap between its two largest
entries ("gap"; a cell whose four entries are all <= 0 carries no gradient: no site, gap = inf).  With `decisions` (a ReLU
keep mask per site group and the arg-max index 0..3 per pool cell) the forward applies them as `h * mask` and a gather
instead of deciding itself, so that autograd gives the gradient UNDER A STATED DECISION PATTERN.  With decisions=None the
operations are the oracle's own, in its order, for any dtype: in float32 this IS the float32 oracle forward.

Site groups: 'encoder.B.1' / 'encoder.B.4' (BatchNorm2d outputs), 'pool.B', '<prefix>.1' (the channel-attention MLP's first
1 x 1 conv, prefix 'attention' or 'channel_attention'), 'classifier.1' / '.5' / '.9' (BatchNorm1d outputs).

Also here: the conditioned cases of tests/golden/train_conditioned.npz (CASES, case_inputs, apply_nudges) shared by the
generator, the host test and the GPU test."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import synthetic_inputs as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "train_conditioned.npz")

# (attention, encoder filters, N): the smallest shapes that reach each path of the trainer (profiles/NOTES_train_conditioned.md)
CASES = (("spatial", (32, 64, 128), 13), ("spatial", (64, 128, 256), 13), ("channel", (64, 128, 256), 13),
         ("none", (128, 256, 512), 13), ("hybrid", (64, 128, 256, 512), 13),
         ("spatial", (32, 64, 128), 3), ("hybrid", (64, 128, 256), 3),
         ("spatial", (64, 128, 256), 16), ("spatial", (32, 64, 128), 33))

# The trainer's hyper-parameter block holds float32 values (LgTrainHparams): the oracle is handed those values, as it is handed
# the float32 parameter values.  With beta2 = 0.999 as a double torch forms 1 - beta2 = 1.0000000e-3; the block's beta2 is
# 0.99900001287..., and 1 - beta2 = 0.99998712e-3: exp_avg_sq would differ by 1.29e-5 relative for this reason alone
# (profiles/NOTES_train_conditioned.md, finding 1).
HPARAMS = {"lr": float(np.float32(0.0005)), "betas": (float(np.float32(0.9)), float(np.float32(0.999))),
           "eps": float(np.float32(1e-8)), "weight_decay": float(np.float32(0.01)), "max_grad_norm": 1.0, "pos_weight": 2.0}


def oracle_step(O, params, x, y, mk, dtype):
    """The oracle's restated step on a case, at the trainer's default hyper-parameters as the device holds them."""
    return O.cnn_train_step(params, x, y, masks=mk, dtype=dtype, **HPARAMS)


def case_tag(att, filt, n):
    return f"{att}_{len(filt)}x{filt[0]}_n{n}"


def case_seed(att, filt, n):
    return 60 + CASES.index((att, tuple(filt), n))


def keep_masks(filt, n, seed):
    """Seeded keep masks scaled by 1 / (1 - p), one per dropout layer (tests/test_gpu_train.py::random_masks)."""
    rng = np.random.default_rng(seed)
    last = filt[-1]                # trainer.dropout_layout restated (asserted equal in the host test)
    layout = [(w, 0.3) for w in filt] + [(last, 0.5), (last // 2, 0.5), (last // 4, 0.4)]
    return [((rng.random((n, w)) >= p) / (1.0 - p)).astype(np.float32) for w, p in layout]


def case_inputs(att, filt, n):
    """Un-nudged float32 parameters, patches, labels and keep masks of a case."""
    seed = case_seed(att, filt, n)
    params = S.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)
    x = S.synthetic_patches(n, seed=seed)
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    return params, x, y, keep_masks(filt, n, seed)


def apply_nudges(params, names, index, delta):
    """The fixture's nudges, added in float32 to copies of the named tensors: p.flat[index] = fl32(p.flat[index] + delta)."""
    out = {k: np.array(v, copy=True) for k, v in params.items()}
    for k, i, d in zip(names, index, delta):
        flat = out[str(k)].reshape(-1)
        flat[int(i)] = np.float32(flat[int(i)] + np.float32(d))
    return out


def conditioned_inputs(fx, att, filt, n):
    tag = case_tag(att, filt, n)
    params, x, y, mk = case_inputs(att, filt, n)
    return apply_nudges(params, fx[f"{tag}_nudge_name"], fx[f"{tag}_nudge_index"], fx[f"{tag}_nudge_delta"]), x, y, mk


def pool_cells(h):
    """[N, C, H, W] -> [N, C, H/2, W/2, 4]: the four entries of every 2 x 2 cell, row-major."""
    n, c, hh, ww = h.shape
    return h.reshape(n, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, hh // 2, ww // 2, 4)


def pool_gap(h):
    """Gap between the two largest entries of every cell of the (post-ReLU) map h; inf where the maximum is not positive."""
    top = pool_cells(h).topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    return torch.where(top[..., 0] > 0, gap, torch.full_like(gap, float("inf")))


def site_groups(params):
    """Names of the site groups in forward order."""
    nb = 0
    while f"encoder.{nb}.0.weight" in params:
        nb += 1
    out = []
    for b in range(nb):
        out += [f"encoder.{b}.1", f"encoder.{b}.4", f"pool.{b}"]
    if "attention.1.weight" in params:
        out.append("attention.1")
    if "channel_attention.1.weight" in params:
        out.append("channel_attention.1")
    return out + ["classifier.1", "classifier.5", "classifier.9"]


def step(params, x, y, masks=None, dtype=torch.float64, decisions=None, pos_weight=2.0, ops=None, want_grads=True):
    """Forward + loss + autograd gradients.  decisions: {'relu': {group: bool array}, 'pool': {group: int array 0..3}} or None.
    ops: {'conv:encoder.B.K' | 'bn:encoder.B.K': callable} replaces that one operation (same signature as F.conv2d(h, w, b,
    padding=1) / F.batch_norm(h, rm, rv, g, b, True, 0.1, 1e-5)): for gradients computed on purpose with a stated defect.
    Returns dict(logits, loss, grads, buffers (running statistics after the step), z, gap, decisions), all numpy."""
    dt = dtype
    ops = ops or {}
    p = {k: torch.as_tensor(np.asarray(v)).to(dt).clone() for k, v in params.items() if not k.endswith("num_batches_tracked")}
    names = [k for k in p if "running_" not in k]
    for k in names:
        p[k].requires_grad_(True)
    h = torch.as_tensor(np.asarray(x)).to(dt)
    yt = torch.as_tensor(np.asarray(y)).to(dt)
    nb = 0
    while f"encoder.{nb}.0.weight" in p:
        nb += 1
    z, gap, taken = {}, {}, {"relu": {}, "pool": {}}
    mi = 0

    def mask():
        nonlocal mi
        mk = None if masks is None else torch.as_tensor(np.asarray(masks[mi])).to(dt)
        mi += 1
        return mk

    def relu(name, h):
        z[name] = h.detach().numpy().astype(np.float64)
        taken["relu"][name] = z[name] > 0
        if decisions is None:
            return F.relu(h)
        return h * torch.as_tensor(np.asarray(decisions["relu"][name])).to(dt)

    def pool(name, h):
        cells = pool_cells(h)
        gap[name] = pool_gap(h.detach()).numpy().astype(np.float64)
        taken["pool"][name] = cells.detach().argmax(dim=-1).numpy()
        if decisions is None:
            return F.max_pool2d(h, 2)
        idx = torch.as_tensor(np.asarray(decisions["pool"][name])).to(torch.int64)
        return torch.gather(cells, -1, idx[..., None])[..., 0]

    for b in range(nb):
        for conv, bn in ((0, 1), (3, 4)):
            cn, bnn = f"encoder.{b}.{conv}", f"encoder.{b}.{bn}"
            h = ops.get("conv:" + cn, F.conv2d)(h, p[cn + ".weight"], p[cn + ".bias"], padding=1)
            h = ops.get("bn:" + bnn, F.batch_norm)(h, p[bnn + ".running_mean"], p[bnn + ".running_var"], p[bnn + ".weight"],
                                                   p[bnn + ".bias"], True, 0.1, 1e-5)
            h = relu(bnn, h)
        h = pool(f"pool.{b}", h)
        mk = mask()
        if mk is not None:
            h = h * mk[:, :, None, None]

    def chan(prefix):
        g = h.mean(dim=(2, 3), keepdim=True)
        a = relu(prefix + ".1", F.conv2d(g, p[prefix + ".1.weight"], p[prefix + ".1.bias"]))
        return torch.sigmoid(F.conv2d(a, p[prefix + ".3.weight"], p[prefix + ".3.bias"]))

    if "attention.0.weight" in p:
        h = h * torch.sigmoid(F.conv2d(h, p["attention.0.weight"], p["attention.0.bias"]))
    elif "attention.1.weight" in p:
        h = h * chan("attention")
    elif "spatial_attention.0.weight" in p:
        sp = torch.sigmoid(F.conv2d(h, p["spatial_attention.0.weight"], p["spatial_attention.0.bias"]))
        h = h * sp * chan("channel_attention")
    h = h.mean(dim=(2, 3))
    for idx in (0, 4, 8):
        bnn = f"classifier.{idx + 1}"
        h = F.linear(h, p[f"classifier.{idx}.weight"], p[f"classifier.{idx}.bias"])
        h = F.batch_norm(h, p[bnn + ".running_mean"], p[bnn + ".running_var"], p[bnn + ".weight"], p[bnn + ".bias"], True, 0.1, 1e-5)
        h = relu(bnn, h)
        mk = mask()
        if mk is not None:
            h = h * mk
    logits = F.linear(h, p["classifier.12.weight"], p["classifier.12.bias"]).reshape(-1)
    loss = F.binary_cross_entropy_with_logits(logits, yt, pos_weight=torch.tensor([float(pos_weight)], dtype=dt))
    out = {"logits": logits.detach().numpy().astype(np.float64), "loss": float(loss.detach()), "z": z, "gap": gap, "decisions": taken,
           "buffers": {k: v.detach().numpy() for k, v in p.items() if "running_" in k}}
    if want_grads:
        gr = torch.autograd.grad(loss, [p[k] for k in names])
        out["grads"] = {k: g.detach().numpy() for k, g in zip(names, gr)}
    return out


def margins(res):
    """Smallest margin per site group: min |z| of a ReLU group, min gap of a pool."""
    out = {k: float(np.abs(v).min()) for k, v in res["z"].items()}
    out.update({k: float(v.min()) for k, v in res["gap"].items()})
    return out


LOCAL = 1e-3      # "local": sites with |z| (or gap) below this in float64


def local_deviation(r32, r64):
    """Per site group, the largest |float32 - float64| of the pre-activation (or pool gap) over the sites whose float64 value is
    below LOCAL.  A group with fewer than 8 such sites (the small late layers) widens the window tenfold until it holds 8
    or every site: the deviation of z = g * (x - mean) / sigma + b is absolute, it does not shrink with |z|."""
    out = {}
    for kind in ("z", "gap"):
        for k, v64 in r64[kind].items():
            a64, a32 = np.abs(v64).reshape(-1), r32[kind][k].reshape(-1)
            fin = np.isfinite(a64) & np.isfinite(a32)
            win = LOCAL
            while (fin & (a64 < win)).sum() < min(8, fin.sum()):
                win *= 10.0
            sel = fin & (a64 < win)
            out[k] = float(np.abs(a32[sel] - v64.reshape(-1)[sel]).max()) if sel.any() else 0.0
    return out


def flip_site(decisions, group, flat_index):
    """A copy of `decisions` with one site decided the other way: a ReLU keep bit toggled, or a pool cell pointed at its
    second-largest entry (given as flat_index = (cell flat index, new arg-max))."""
    out = {"relu": {k: v.copy() for k, v in decisions["relu"].items()}, "pool": {k: v.copy() for k, v in decisions["pool"].items()}}
    if group.startswith("pool."):
        cell, arg = flat_index
        out["pool"][group].reshape(-1)[cell] = arg
    else:
        flat = out["relu"][group].reshape(-1)
        flat[flat_index] = ~flat[flat_index]
    return out


def yardstick_quantities(r, ref):
    """Deviations of one oracle-style result dict `r` (cnn_train_step's layout, or the device's values arranged the same way)
    from the float64 result `ref`: the quantities the conditioned GPU test bounds, in one flat dict of floats."""
    out = {"loss": abs(r["loss"] - ref["loss"]), "grad_norm": abs(r["grad_norm"] - ref["grad_norm"]),
           "logits": float(np.abs(np.asarray(r["logits"], np.float64) - ref["logits"]).max())}
    for k, g in ref["grads"].items():
        d = np.asarray(r["grads"][k], np.float64) - g
        den = float(np.linalg.norm(g))
        out["grad_l2/" + k] = float(np.linalg.norm(d)) / den if den > 0 else 0.0
        out["grad_max/" + k] = float(np.abs(d).max())
    for k, v in ref["params"].items():
        if "running_" in k:
            out["buffer/" + k] = float(np.abs(np.asarray(r["params"][k], np.float64) - v).max())
    for key, short in (("exp_avg", "m"), ("exp_avg_sq", "v")):
        for k, v in ref["opt_state"][key].items():
            out[f"{short}/{k}"] = float(np.abs(np.asarray(r["opt_state"][key][k], np.float64) - v).max())
    return out


ULP32 = 2.0 ** -23


def floors(ref):
    """4 float32 ulps of the largest entry of the tensor a quantity is taken on (relative L2: 4 ulps relative, which is
    what a tensor whose every element is 4 of its own ulps off can reach)."""
    def ulps(v):
        m = float(np.abs(np.asarray(v, np.float64)).max())
        return 4.0 * float(np.spacing(np.float32(m))) if m > 0 else 0.0
    out = {"loss": ulps(ref["loss"]), "grad_norm": ulps(ref["grad_norm"]), "logits": ulps(ref["logits"])}
    for k, g in ref["grads"].items():
        out["grad_l2/" + k] = 4.0 * ULP32
        out["grad_max/" + k] = ulps(g)
    for k, v in ref["params"].items():
        if "running_" in k:
            out["buffer/" + k] = ulps(v)
    for key, short in (("exp_avg", "m"), ("exp_avg_sq", "v")):
        for k, v in ref["opt_state"][key].items():
            out[f"{short}/{k}"] = ulps(v)
    return out


def zero_gradient(ref, k):
    """compare_step's rule for a bias in front of a BatchNorm (mathematically zero gradient; tests/test_gpu_train.py)."""
    return float(np.linalg.norm(ref["grads"][k])) < 1e-4 * ref["grad_norm"] / np.sqrt(len(ref["grads"]))


BOUND_FACTOR = 4.0      # the factor the optimiser tests use (profiles/NOTES_train_tests.md)
# The head: single numbers, and the tensors whose gradient is a sum over the batch of d loss / d logit (or one step from it).
# Each is a direct function of the N logit errors, |d q| <= sum_i |dq / dz_i| |dz_i|, so a device whose logits sit inside their
# own bound can be several times torch's yardstick of q off, and the yardstick of a single number is a single draw.  Measured
# on the device at most 8.3 x; lgt_conv_kernel's one-chain float32 sum emulated on the CPU gives the same picture
# (tests/tools/train_conditioned_orders.py; profiles/NOTES_train_conditioned.md, finding 2).  16 is the most a factor may be.
HEAD_FACTOR = 16.0
# exp_avg_sq = (1 - beta2) g'^2 deviates by 2 g' dg': its largest deviation sits on a large gradient element, the gradient's own
# anywhere, so the two yardsticks are drawn on different elements and a gradient inside its bound (measured up to 0.91 of it)
# leaves exp_avg_sq at up to 4.7 x its yardstick; same emulation, same notes (finding 3).
SQUARE_FACTOR = 8.0
HEAD_QUANTITIES = ("loss", "grad_norm")


def head_tensors(ref):
    return {k for k, g in ref["grads"].items() if k.startswith("classifier.12.") or g.size == 1}


def factor(k, ref):
    if k in HEAD_QUANTITIES or k.partition("/")[2] in head_tensors(ref):
        return HEAD_FACTOR
    return SQUARE_FACTOR if k.startswith("v/") else BOUND_FACTOR


def bounds(fx, tag, ref):
    """Per quantity: factor x the fixture's yardstick (float32 oracle against float64 oracle on this case, the maximum over 1, 2
    and 8 threads), floored at 4 float32 ulps of the tensor's largest entry.  factor = 4; exp_avg_sq 8; the head 16."""
    yard = dict(zip((str(k) for k in fx[f"{tag}_yard_key"]), (float(v) for v in fx[f"{tag}_yard"])))
    fl = floors(ref)
    assert set(yard) == set(fl)
    return {k: max(factor(k, ref) * yard[k], fl[k]) for k in yard}
