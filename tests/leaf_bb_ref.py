"""The list filter of the clutter arg-max's branch-and-bound pass (lg_leaf.hip::k_edt_bb) restated in NumPy / SciPy: does a
leaf mask overflow a survivor list, i.e. does the full-transform fallback run?  The device evaluates cell centres exactly
unless the cell is already lost, so exact centre values from scipy's transform give the same survivors."""
import numpy as np
from scipy import ndimage

CAP = 65536 // 4   # LGL_QCAP / 4: every survivor has four children


def exact_field(leaf):
    """Euclidean distance of every pixel to the nearest leaf pixel (float64), as the oracle's clutter field.  Without a leaf
    pixel the distance is infinite everywhere (scipy's transform has no defined answer there): a constant field, whose
    arg-extrema are index 0, which is what the library reports for such a frame."""
    leaf = np.asarray(leaf, bool)
    return ndimage.distance_transform_edt(~leaf) if leaf.any() else np.full(leaf.shape, np.inf)


def _centres(y0, x0, s, H, W):
    y1, x1 = np.minimum(y0 + s, H) - 1, np.minimum(x0 + s, W) - 1      # last pixel of the cell inside the image
    cy, cx = np.minimum(y0 + s // 2, y1), np.minimum(x0 + s // 2, x1)
    ry, rx = np.maximum(cy - y0, y1 - cy), np.maximum(cx - x0, x1 - cx)
    return cy, cx, np.sqrt((ry * ry + rx * rx).astype(np.float64))


def bb_survivors(leaf):
    """-> [(cell size, survivors)] level by level, until the first list that overflows or cells of one pixel."""
    leaf = np.asarray(leaf, bool)
    H, W = leaf.shape
    if not leaf.any() or leaf.all():
        return []                                                        # constant field: the pass answers at once
    d2 = np.rint(exact_field(leaf) ** 2).astype(np.int64)
    S = 64
    while -(-H // S) * -(-W // S) > 8192:
        S *= 2
    y0, x0 = [a.ravel() for a in np.meshgrid(np.arange(0, H, S), np.arange(0, W, S), indexing="ij")]
    best, levels = 0, []
    while True:
        cy, cx, rad = _centres(y0, x0, S, H, W)
        v = d2[cy, cx]
        best = max(best, int(v.max()))                                   # best value so far: every centre evaluated
        keep = np.sqrt(v.astype(np.float64)) + rad + 1e-6 >= np.sqrt(float(best))
        levels.append((S, int(keep.sum())))
        if keep.sum() > CAP or S == 1:
            return levels
        S //= 2
        y0 = (y0[keep][:, None] + np.array([0, 0, S, S])).ravel()
        x0 = (x0[keep][:, None] + np.array([0, S, 0, S])).ravel()
        inside = (y0 < H) & (x0 < W)
        y0, x0 = y0[inside], x0[inside]


def bb_overflows(leaf):
    lv = bb_survivors(leaf)
    return bool(lv) and lv[-1][1] > CAP


# ---------------------------------------------------------------------------------------------- masks that force the fallback
# A pitch-2 lattice of leaf pixels: the field is at most sqrt(2) away from the lattice, every cell of 2 x 2 pixels has a centre
# value of 2 and a half diagonal of sqrt(2), so while the best value stays <= 8 every such cell survives: ceil(H / 2) *
# ceil(W / 2) survivors.  One shape per instantiation of the fallback's row kernel (padded widths 512 .. 4096) and 18 x 4096,
# the widest frame the stage takes.
FALLBACK_SHAPES = {(258, 256): 16512, (130, 520): 16900, (66, 1030): 16995, (34, 2050): 17425, (18, 4096): 18432}


def lattice(H, W, holes=()):
    m = np.zeros((H, W), np.int16)
    m[::2, ::2] = 1
    for (y, x) in holes:
        assert m[y, x] == 1, (y, x)
        m[y, x] = 0
    return m


def batch_frames():
    """-> ([ordinary scene, lattice with holes, empty, all leaf, sparse specks] at 130 x 520, the scene's depth): only the
    second overflows."""
    from synthetic_inputs import synthetic_scene

    H, W = 130, 520
    scene, depth, _ = synthetic_scene(H, W, 6)
    specks = np.zeros((H, W), np.int16)
    specks[np.random.default_rng(17).random((H, W)) > 0.999] = 4
    return [scene, lattice_variants(H, W)["holes"][0], np.zeros((H, W), np.int16), np.ones((H, W), np.int16), specks], depth


def wide_masks(H, W):
    """Sparse masks around the first and the last 64-bit word of a bit row (W > 4032: the last word is the 64th), label 1."""
    last = 64 * ((W - 1) // 64)                                              # first column of the row's last word
    rng = np.random.default_rng(23)
    out = {}
    m = np.zeros((H, W), np.int16); m[rng.integers(0, H, 12), rng.integers(0, 64, 12)] = 1; out["first_word_only"] = m
    m = np.zeros((H, W), np.int16); m[rng.integers(0, H, 12), rng.integers(last, W, 12)] = 1; out["last_word_only"] = m
    m = np.zeros((H, W), np.int16); m[20, W - 1] = 1; out["last_pixel"] = m
    m = np.zeros((H, W), np.int16); m[7, 5] = 1; m[31, W - 1] = 1; out["first_and_last_word"] = m
    return out


def wide_noise():
    return (np.random.default_rng(31).random((64, 3840)) > 0.5).astype(np.int16)


def lattice_variants(H, W):
    """-> {name: (mask, expected arg-max or None)} -- H and W even: the last lattice row / column is H - 2 / W - 2, and a hole
    there leaves a pixel of the frame's last row / column at d2 = 5 where a hole elsewhere gives 4 and the lattice itself 2."""
    r, lc, lr = (H // 4) * 2, W - 2, H - 2
    return {
        "holes": (lattice(H, W, [(r, 64), (r, lc)]), (r, W - 1)),             # unique maximum in the frame's last column
        "hole_col0": (lattice(H, W, [(r, 0)]), (r, 0)),                       # position 0 of a row
        "hole_row0": (lattice(H, W, [(0, 66)]), (0, 66)),
        "hole_last_row": (lattice(H, W, [(lr, 66)]), (H - 1, 66)),
        "hole_first_and_last_row": (lattice(H, W, [(0, 66), (lr, 130)]), (H - 1, 130)),
        "two_holes_tie": (lattice(H, W, [(r + 4, lc), (r - 2, lc)]), (r - 2, W - 1)),   # the first in row-major order
        "plain": (lattice(H, W), (1, 1)),                                     # thousands of ties
    }
