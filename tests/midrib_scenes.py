"""Seeded RGB leaf scenes for the detect_midrib tests: an elliptical leaf with a brighter ridge along its major axis, on a
noisy background.  kind: "leaf", "empty" (no mask), "thin" (minor axis < 6), "edge" (the leaf runs off the frame)."""
import numpy as np


def leaf_scene(H, W, rng, kind="leaf"):
    img = rng.integers(0, 70, (H, W, 3), dtype=np.int32)
    mask = np.zeros((H, W), np.uint8)
    if kind == "empty":
        return mask, img.astype(np.uint8)
    s = min(H, W)
    theta = rng.uniform(0.0, np.pi)
    if kind == "thin":
        a, b = rng.uniform(4.0, 12.0), rng.uniform(0.6, 2.2)
    else:
        a = rng.uniform(0.15, 0.4) * s
        b = a * rng.uniform(0.25, 0.55)
    if kind == "edge":
        cx = rng.choice([rng.uniform(-0.1 * a, 0.3 * a), rng.uniform(W - 0.3 * a, W + 0.1 * a)])
        cy = rng.uniform(0.2 * H, 0.8 * H)
    else:
        cx = rng.uniform(a + 2, W - a - 2) if W > 2 * a + 4 else W / 2
        cy = rng.uniform(a + 2, H - a - 2) if H > 2 * a + 4 else H / 2
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (xx - cx) * np.cos(theta) + (yy - cy) * np.sin(theta)
    v = -(xx - cx) * np.sin(theta) + (yy - cy) * np.cos(theta)
    inside = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    mask[inside] = 1
    leaf = np.stack([rng.integers(20, 70, (H, W)), rng.integers(90, 170, (H, W)), rng.integers(20, 70, (H, W))], -1)
    ridge = np.abs(v) < max(1.0, 0.1 * b)
    leaf[ridge] += np.array([50, 70, 50])
    img = np.where(inside[..., None], leaf, img)
    return mask, np.clip(img, 0, 255).astype(np.uint8)


def scene_batch(B, H, W, seed, kinds=("leaf", "leaf", "edge", "thin", "empty")):
    rng = np.random.default_rng(seed)
    ms, ims = [], []
    for i in range(B):
        m, im = leaf_scene(H, W, rng, kinds[i % len(kinds)])
        ms.append(m)
        ims.append(im)
    return np.stack(ms), np.stack(ims)
