"""The fold reference (tests/cnn_fold_ref.py) against first principles, in float64 on the CPU: it is the witness of the weight
bits in tests/test_gpu_device_eval.py, so it is proved here on its own.

Seeded tensors with one block's worth of channels (9 -> 16 -> 16).  Tolerances are those of float64 arithmetic: sums of at
most 16 * 9 products of O(1) numbers carry ~1e-14 relative error, so 1e-12 relative for the fold; the F(4x4) transforms
multiply by up to 8 * 8 and 5 * 5 before the sum cancels, 1e-10 for the Winograd identity."""
import numpy as np
import pytest

from tests import cnn_fold_ref as R

torch = pytest.importorskip("torch")

EPS = float(R.EPS)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)


def conv_layer(rng, cin, cout):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(w=f(cout, cin, 3, 3) * 0.3, b=f(cout), g=rng.uniform(0.5, 1.5, cout).astype(np.float32), beta=f(cout),
                mean=f(cout) * 0.5, var=rng.uniform(0.5, 2.0, cout).astype(np.float32))


LAYERS = [(9, 16, 10, 64), (16, 16, 64, 64)]   # cnn_fold_ref.layer_plan((16,))


@pytest.fixture(scope="module")
def folded():
    rng = np.random.default_rng(11)
    out = []
    for cin, cout, _, _ in LAYERS:
        p = conv_layer(rng, cin, cout)
        out.append((p, *R.fold_conv(p["w"], p["b"], p["g"], p["beta"], p["mean"], p["var"])))
    return out


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_layer_plan():
    assert R.layer_plan((16,)) == LAYERS
    assert R.layer_plan((32, 64, 128))[:3] == [(9, 32, 10, 64), (32, 32, 64, 64), (32, 64, 64, 64)]


def test_folded_conv_equals_batchnorm_of_conv(folded):
    rng = np.random.default_rng(12)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    for p, wf, bf in folded:
        x = rng.standard_normal((2, wf.shape[1], 8, 8))
        y = torch.nn.functional.conv2d(t(x), t(p["w"]), t(p["b"]), padding=1)
        ref = torch.nn.functional.batch_norm(y, t(p["mean"]), t(p["var"]), t(p["g"]), t(p["beta"]), training=False, eps=EPS)
        got = torch.nn.functional.conv2d(t(x), t(wf), t(bf), padding=1)
        assert rel(got.numpy(), ref.numpy()) <= 1e-12


def test_folded_classifier_equals_batchnorm_of_linear():
    rng = np.random.default_rng(13)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    w, b, g, beta, mean, var = f(8, 16) * 0.3, f(8), rng.uniform(0.5, 1.5, 8).astype(np.float32), f(8), f(8), \
        rng.uniform(0.5, 2.0, 8).astype(np.float32)
    x = rng.standard_normal((5, 16))
    wt, bt = R.fold_fc(w, b, g, beta, mean, var)
    ref = torch.nn.functional.batch_norm(torch.nn.functional.linear(t(x), t(w), t(b)), t(mean), t(var), t(g), t(beta),
                                         training=False, eps=EPS)
    assert rel(x @ wt.T + bt, ref.numpy()) <= 1e-12
    wt, bt = R.fold_fc(w, b)     # the last layer: no BatchNorm1d
    assert np.array_equal(wt, w.astype(np.float64)) and np.array_equal(bt, b.astype(np.float64))


@pytest.mark.parametrize("name,bt,at,m", [("wino2", BT2, AT2, 2), ("wino4", BT4, AT4, 4)])
def test_winograd_weights_reproduce_the_direct_convolution(folded, name, bt, at, m):
    rng = np.random.default_rng(14)
    for _, wf, _ in folded:
        cout, cin = wf.shape[:2]
        u = getattr(R, name)(wf)                                   # [co][ci][m+2][m+2], not rounded
        d = rng.standard_normal((cin, m + 2, m + 2))
        v = bt @ d @ bt.T                                          # [ci][m+2][m+2]
        got = at @ (u * v[None]).sum(axis=1) @ at.T                # [co][m][m]
        ref = np.zeros((cout, m, m))
        for y in range(m):
            for x in range(m):
                ref[:, y, x] = (wf * d[None, :, y:y + 3, x:x + 3]).sum(axis=(1, 2, 3))
        assert rel(got, ref) <= 1e-10


def test_unpacking_returns_the_tensor_and_padding_is_zero(folded):
    for L, ((_, wf, _), (cin, cout, cinp, coutp)) in enumerate(zip(folded, LAYERS)):
        cases = [(wf.reshape(cout, cin, 9), R.pack_direct(wf, cinp, coutp), R.unpack_direct, cinp),
                 (R.wino2(wf).reshape(cout, cin, 16), R.pack_wino2(R.wino2(wf), cinp if L else 12, coutp), R.unpack_wino2, cinp if L else 12),
                 (R.wino4(wf).reshape(cout, cin, 36), R.pack_wino4(R.wino4(wf), cinp if L else 12, coutp), R.unpack_wino4, cinp if L else 12)]
        for tensor, flat, unpack, ci_pad in cases:
            assert flat.size == tensor.shape[2] * ci_pad * coutp
            full = unpack(flat, ci_pad, coutp)
            assert full.shape == (coutp, ci_pad, tensor.shape[2])
            assert np.array_equal(full[:cout, :cin], tensor)
            assert not full[cout:].any() and not full[:, cin:].any()
            assert np.count_nonzero(flat) == np.count_nonzero(tensor)


def test_reference_buffers_of_a_state_dict():
    """Sizes, the buffers a model has, and the single rounding: every float32 is the nearest to the float64 it came from."""
    import synthetic_inputs as S
    for filt in ((64, 128, 256), (32, 64, 128)):
        state = S.cnn_closed_form_params(seed=1, attention_type="none", filters=filt)
        ref = R.fold_reference(state)
        plan = R.layer_plan(filt)
        for L, (cin, cout, cinp, coutp) in enumerate(plan):
            assert ref["bconv", L].size == coutp and ref["uwino4", L].size == 36 * (12 if L == 0 else cinp) * coutp
            assert (("wconv", L) in ref) == (L == 0 or filt == (64, 128, 256)) and (("uwino", L) in ref) == (L >= 1)
        F = filt[-1]
        assert [ref["fcw", k].size for k in range(4)] == [F * F, F * F // 2, F * F // 8, F // 4]
        assert all(v.dtype == np.float32 for v in ref.values())
        wf, bf = R.fold_conv(*[state[f"encoder.0.{k}"] for k in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean",
                                                                  "1.running_var")])
        assert np.array_equal(R.unpack_direct(ref["wconv", 0], 10, plan[0][3])[:filt[0], :9].reshape(filt[0], 9, 3, 3),
                              wf.astype(np.float32))
        assert np.array_equal(ref["bconv", 0][:filt[0]], bf.astype(np.float32))
