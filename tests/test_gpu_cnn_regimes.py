"""The CNN at every work plan the F(4x4,3x3) launcher can make, against the float64 reference network.

tests/cnn_plan.py restates launch_wino4_rt's plan (full rounds R, left-over items rem, the split P of a left-over item over
2, 4 or 8 workgroups) and picks, for every layer of the model under test, the smallest patch count of every plan class the
device's CU count reaches, plus one frame, config 3, the headline's 5120 patches and the slice boundary at 8192.  Left-over
items compute the HIGHEST patch indices of a batch, so every logit of every count is checked, not a prefix.

Batch position i holds patch i % M of a pool of M distinct patches; M is prime so that an addressing error of one period
cannot map a patch onto a copy of itself."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import lg_oracle as O  # noqa: E402
from tests import cnn_plan as C  # noqa: E402
from tests.test_gpu_parity import _wide_range_params  # noqa: E402

M = 2053          # distinct patches of the standard model's pool (a prime above 2048)
M_VAR = 509       # the variants' pool (a prime near 512: bounds the float64 cost of the wider encoders)
RTOL, ATOL = 1e-4, 1e-5         # against float64 (test_cnn_vs_reference_golden)
SRTOL, SATOL = 1e-5, 1e-6       # the same patch in another position or batch: summation order only
STANDARD = (64, 128, 256)
VARIANTS = {   # name: (seed, attention, encoder filters), as test_cnn_attention_variants_vs_reference
    "channel": (1, "channel", STANDARD), "hybrid": (1, "hybrid", STANDARD), "none": (1, "none", STANDARD),
    "lightweight": (2, "spatial", (32, 64, 128)), "deep": (2, "hybrid", (64, 128, 256, 512)),
    "wide": (2, "none", (128, 256, 512)),
}


@pytest.fixture(scope="module")
def sel():
    import leafgrasp_amd

    assert torch.cuda.is_available()
    s = leafgrasp_amd.GraspPointSelector(torch.device("cuda:0"), load_model=False)
    yield s
    s.clear_cnn()


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


@functools.lru_cache(maxsize=None)
def _pool(m, seed):
    return O.synthetic_patches(m, seed=seed)


@functools.lru_cache(maxsize=None)
def _pool_dev(m, seed):
    return torch.from_numpy(_pool(m, seed)).cuda()


@functools.lru_cache(maxsize=None)
def _params(name):
    if name == "standard":
        return O.cnn_closed_form_params(seed=0)
    if name == "wide_range":
        return _wide_range_params(0)
    seed, att, filt = VARIANTS[name]
    return O.cnn_closed_form_params(seed=seed, attention_type=att, filters=filt)


@functools.lru_cache(maxsize=None)
def _ref(name, m, seed):
    """float64 logits of the pool under the named parameters."""
    return O.cnn_forward(_params(name), _pool(m, seed), dtype=torch.float64)


def _run(sel, pool, n):
    idx = torch.arange(n, device=pool.device) % pool.shape[0]
    return sel.cnn_forward(pool[idx]).cpu().numpy()


def _check_counts(sel, pool, ref, base, counts, what):
    """Every logit of every count against float64 and against the pool's own logits; a repeated call bit for bit."""
    m = pool.shape[0]
    for n in counts:
        got = _run(sel, pool, n)
        idx = np.arange(n) % m
        np.testing.assert_allclose(got, ref[idx], rtol=RTOL, atol=ATOL, err_msg=f"{what}: N {n} against float64")
        np.testing.assert_allclose(got, base[idx], rtol=SRTOL, atol=SATOL, err_msg=f"{what}: N {n} against the pool's logits")
        np.testing.assert_array_equal(_run(sel, pool, n), got, err_msg=f"{what}: N {n}, second call")


def test_plan_table_reaches_every_class(num_cu):
    layers = C.model_layers(STANDARD)
    counts, first = C.pick_counts(layers, num_cu)
    print()
    print(C.table(layers, counts, num_cu))
    hit = C.hit_classes(layers, counts, num_cu)
    for (li, c), n in first.items():
        print(f"L{li} {C.class_name(c):16s} first at N {n:5d}: {'hit' if (li, c) in hit else 'MISSED'}")
    assert set(first) <= hit
    classes = {c for _, c in first}
    if num_cu == 256:   # the MI355X: every class the kernel has -- split items before and after full rounds, P = 2, 4, 8
        assert classes == {(False, True, 8), (False, True, 4), (False, True, 2), (True, False, 1), (True, True, 1),
                           (True, True, 2), (True, True, 4), (True, True, 8)}, sorted(classes)


def test_standard_model_at_every_plan(sel, num_cu):
    counts, _ = C.pick_counts(C.model_layers(STANDARD), num_cu)
    pool = _pool_dev(M, 31)
    ref = _ref("standard", M, 31)
    sel.set_cnn_state_dict(_params("standard"))
    base = _run(sel, pool, M)
    np.testing.assert_allclose(base, ref, rtol=RTOL, atol=ATOL, err_msg=f"N {M}")
    _check_counts(sel, pool, ref, base, counts, "standard")
    sel.clear_cnn()


def test_slices_of_8192(sel):
    """8193 patches run as a slice of 8192 and a slice of one: each equals its own call bit for bit."""
    pool = _pool_dev(M, 31)
    ref = _ref("standard", M, 31)
    sel.set_cnn_state_dict(_params("standard"))
    got = _run(sel, pool, 8193)
    np.testing.assert_array_equal(got[:8192], _run(sel, pool, 8192))
    lone = 8192 % M
    one = sel.cnn_forward(pool[lone:lone + 1]).cpu().numpy()
    np.testing.assert_array_equal(got[8192:], one)
    np.testing.assert_allclose(got[8192], ref[lone], rtol=RTOL, atol=ATOL)
    sel.clear_cnn()


FORMS = [("direct", {"LG_CNN_DIRECT": "1"}), ("f23", {"LG_CNN_F23": "1"})] + \
        [(f"wino_mask_{b}", {"LG_CNN_WINO_MASK": str(b)}) for b in (1, 2, 4, 8, 16, 32, 0x3f)]


def _load_with_env(sel, monkeypatch, params, env):
    """The switches are read when the model is loaded (lg_cnn_load)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sel.set_cnn_state_dict(params)
    for k in env:
        monkeypatch.delenv(k)


@pytest.mark.parametrize("form,env", FORMS, ids=[f for f, _ in FORMS])
def test_conv_forms_against_float64(sel, monkeypatch, form, env):
    pool = _pool_dev(M, 31)
    ref = _ref("standard", M, 31)
    _load_with_env(sel, monkeypatch, _params("standard"), env)
    for n in (20, 640, 5121):
        got = _run(sel, pool, n)
        np.testing.assert_allclose(got, ref[np.arange(n) % M], rtol=RTOL, atol=ATOL, err_msg=f"{form}: N {n}")
    sel.clear_cnn()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_at_every_plan(sel, num_cu, name):
    layers = C.model_layers(VARIANTS[name][2])
    counts, first = C.pick_counts(layers, num_cu)
    assert set(first) <= C.hit_classes(layers, counts, num_cu)
    pool = _pool_dev(M_VAR, 32)
    ref = _ref(name, M_VAR, 32)
    sel.set_cnn_state_dict(_params(name))
    base = _run(sel, pool, M_VAR)
    np.testing.assert_allclose(base, ref, rtol=RTOL, atol=ATOL, err_msg=f"{name}: N {M_VAR}")
    _check_counts(sel, pool, ref, base, counts, name)
    sel.clear_cnn()


@pytest.mark.parametrize("form,env", [("direct", {"LG_CNN_DIRECT": "1"}), ("f23", {"LG_CNN_F23": "1"}), ("f43", {})],
                         ids=["direct", "f23", "f43"])
def test_wide_range_weights_at_the_split_plans(sel, monkeypatch, num_cu, form, env):
    """_wide_range_params(0) (BN-folded per-channel scales from 0.25 to 40) at every count whose plan splits a left-over item
    over 8 or 4 workgroups, and at 5121: max |err| / max |logit| <= 1e-4."""
    _, first = C.pick_counts(C.model_layers(STANDARD), num_cu)
    counts = sorted({n for (_, c), n in first.items() if c[2] in (4, 8)} | {5121})
    pool = _pool_dev(M_VAR, 33)
    ref = _ref("wide_range", M_VAR, 33)
    scale = float(np.abs(ref).max())
    _load_with_env(sel, monkeypatch, _params("wide_range"), env)
    errs = {}
    for n in counts:
        got = _run(sel, pool, n)
        errs[n] = float(np.abs(got - ref[np.arange(n) % M_VAR]).max() / scale)
    print(f"wide-range {form}: max |err| / max |logit| per N:", errs, "max |logit|", scale)
    sel.clear_cnn()
    assert all(e <= 1e-4 for e in errs.values()), errs
