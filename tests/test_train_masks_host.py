"""CPU properties of the restated dropout-mask draw (tests/train_masks_ref.py), the specification that
tests/test_gpu_train_masks.py holds lgt_mask_kernel to bit for bit."""
import numpy as np
import pytest

from leafgrasp_amd.trainer import dropout_layout
from tests import train_masks_ref as R


COMBOS = [(42, 0, 16), (42, 1, 16), (7, 5, 13), (42, 0, 2)]
ENCODERS = [(64, 128, 256), (32, 64, 128), (64, 128, 256, 512)]


@pytest.mark.parametrize("filt", ENCODERS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("seed,step,n", COMBOS)
def test_keep_rate_and_values(seed, step, n, filt):
    lay = dropout_layout(filt)
    mk = R.masks(seed, step, n, lay)
    assert len(mk) == len(lay)
    for m, (w, p) in zip(mk, lay):
        assert m.shape == (n, w) and m.dtype == np.float32
        kv = R.keep_value(p)
        assert kv.dtype == np.float32
        assert np.all((m == 0) | (m == kv))                       # exactly 0 or the float32 keep value
        cnt = n * w
        sigma = np.sqrt(p * (1.0 - p) / cnt)                      # binomial sigma of the keep rate
        dev = abs(float((m != 0).mean()) - (1.0 - p)) / sigma
        assert dev <= 4.5, (w, p, dev)


def test_keep_value_is_float32_arithmetic():
    # 1 / (1 - 0.3f) in float32 is not float32(1 / 0.7): the mask value is the former
    assert R.keep_value(0.3) == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.3))
    assert R.keep_value(0.5) == np.float32(2.0)
    assert float(R.keep_value(0.4)) == pytest.approx(1.0 / 0.6, rel=2e-7)


def test_uniforms_are_24_bit_and_wrap_in_uint64():
    """A seed above 2^32 makes seed * 0x100000001B3 exceed 2^64: the result must equal the one computed entry by entry with
    Python integers reduced mod 2^64."""
    seed, step, cnt = (1 << 33) + 12345, 3, 64
    u = R.uniforms(seed, step, cnt)
    m = (1 << 64) - 1
    s = (seed * 0x100000001B3 + 0x51 * step) & m
    for i in range(cnt):
        z = (s + 0x9E3779B97F4A7C15 * (i + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        assert float(u[i]) == (z >> 40) / 16777216.0
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0


@pytest.mark.parametrize("filt", ENCODERS, ids=lambda f: "x".join(map(str, f)))
def test_masks_vary_with_step_and_seed(filt):
    lay = dropout_layout(filt)
    flat = lambda seed, step: np.concatenate([m.reshape(-1) for m in R.masks(seed, step, 16, lay)])  # noqa: E731
    a = flat(42, 0)
    for other in (flat(42, 1), flat(43, 0)):
        assert float((a != other).mean()) > 0.30
    np.testing.assert_array_equal(a, flat(42, 0))
