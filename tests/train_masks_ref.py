"""NumPy restatement of the device-drawn dropout keep masks of the trainer (include/leafgrasp.h: masks = NULL, "drawn on the
device from `seed` and the step counter"; lgt_mask_kernel in lg_train_optim.hip).

One counter-based hash per mask entry.  The entries of all dropout layers form one flat vector laid out [layer][N][width]
in dropout_layout(filters) order; entry i (0-based) gets

    s  = seed * 0x100000001B3 + 0x51 * step                       (mod 2^64)
    z  = s + 0x9E3779B97F4A7C15 * (i + 1)                         (mod 2^64)
    z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31      (splitmix64)
    u  = float32(z >> 40) * 2^-24                                 (24 random bits: exact in float32)
    mask = 1 / (1 - p) if u >= p else 0                           (float32 arithmetic, p the layer's float32 drop rate)

`step` is the optimizer's step count BEFORE the step that draws the masks (0 for a fresh trainer).  Every product wraps in
uint64: the scalar part is computed with Python integers and reduced mod 2^64, the per-entry part on uint64 ARRAYS (NumPy
wraps those silently; uint64 SCALARS would raise overflow warnings and, mixed with Python ints, turn into float64)."""
import numpy as np

_M64 = (1 << 64) - 1


def keep_value(p):
    """float32(1) / (float32(1) - float32(p)), rounded once more to float32 -- the kernel's `1.0f / (1.0f - p)`."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def uniforms(seed, step, count):
    """The `count` float32 uniforms in [0, 1) of flat entries 0 .. count-1."""
    s = (int(seed) * 0x100000001B3 + 0x51 * int(step)) & _M64
    z = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.full(count, s, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    assert z.dtype == np.uint64
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def masks(seed, step, n, layout):
    """layout: [(width, p)] as leafgrasp_amd.trainer.dropout_layout gives it.  Returns one float32 [n, width] keep mask
    per dropout layer, in that order."""
    u = uniforms(seed, step, n * sum(w for w, _ in layout))
    out, o = [], 0
    for w, p in layout:
        blk = u[o:o + n * w].reshape(n, w)
        out.append(np.where(blk >= np.float32(p), keep_value(p), np.float32(0.0)).astype(np.float32))
        o += n * w
    return out
