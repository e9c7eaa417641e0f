"""numpy restatement of the near-tile predicate of the score-plane kernel (lg_final_kernel), tile by tile, for the tests of the
near launch: a 64 x 16 tile at (tx0, ty0) looks at the mask (bit-row test) on columns tx0-8 .. tx0+71 and on rows ty0-HALO ..
ty0+15+HALO reflected at the frame border, and can only meet the mask when

    bx1 >= bx0 and bx0 <= tx0 + 71 and bx1 >= tx0 - 8 and by0 <= ty0 + 15 + HALO and by1 >= ty0 - 16 - HALO

for the mask's bounding box [bx0, bx1] x [by0, by1].  The library states this once (lg_near_tiles in lg_planes.h, exported as
lg_near_tile_rect); nothing here calls it."""
import numpy as np

TW, TH = 64, 16


def tile_grid(H, W):
    return (W + TW - 1) // TW, (H + TH - 1) // TH


def near_map(box, H, W, halo):
    """bool [tiles_y, tiles_x]: the per-tile expression, evaluated for every tile on its own"""
    bx0, bx1, by0, by1 = box
    tiles_x, tiles_y = tile_grid(H, W)
    out = np.zeros((tiles_y, tiles_x), bool)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tx0, ty0 = tx * TW, ty * TH
            out[ty, tx] = (bx1 >= bx0 and bx0 <= tx0 + TW + 7 and bx1 >= tx0 - 8 and by0 <= ty0 + TH - 1 + halo
                           and by1 >= ty0 - TH - halo)
    return out


def near_map_grid(xs, ys, H, W, halo):
    """the same expression for every box (xs[i], xs[j], ys[k], ys[l]) at once: the column half [i, j, tx] and the row half
    [k, l, ty] of the conjunction (a tile is near when both hold and the box is not empty)"""
    tiles_x, tiles_y = tile_grid(H, W)
    xs, ys = np.asarray(xs), np.asarray(ys)
    tx0 = np.arange(tiles_x) * TW
    ty0 = np.arange(tiles_y) * TH
    bx0, bx1 = xs[:, None, None], xs[None, :, None]
    by0, by1 = ys[:, None, None], ys[None, :, None]
    colh = (bx1 >= bx0) & (bx0 <= tx0 + TW + 7) & (bx1 >= tx0 - 8)
    rowh = (by0 <= ty0 + TH - 1 + halo) & (by1 >= ty0 - TH - halo)
    return colh, rowh


def rect_of(near):
    """(tx_lo, tx_hi, ty_lo, ty_hi), count of a near map; asserts that the near tiles are exactly a rectangle"""
    if not near.any():
        return (0, -1, 0, -1), 0
    ys, xs = np.nonzero(near)
    r = (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))
    assert near[r[2]:r[3] + 1, r[0]:r[1] + 1].all()
    return r, int(near.sum())


def bbox(mask):
    """bounding box of a 2-D mask as the library keeps it: (bx0, bx1, by0, by1), (0, -1, 0, -1) when it is empty"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return (0, -1, 0, -1)
    return (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))


def near_offsets(masks, halo):
    """what lg_debug_near_tiles returns for a batch of masks [B, H, W]: the exclusive scan of the frames' near counts, B + 1"""
    H, W = masks.shape[1:]
    counts = [int(near_map(bbox(m), H, W, halo).sum()) for m in masks]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def reflect(v, n):
    """lg_reflect: torch's 'reflect' index, clamped"""
    v = np.abs(np.asarray(v))
    v = np.where(v >= n, 2 * (n - 1) - v, v)
    return np.clip(v, 0, n - 1)


def reach_map(mask, halo):
    """bool [tiles_y, tiles_x]: tiles whose bit-row test finds a mask bit -- rows lg_reflect(ty0-halo .. ty0+15+halo), columns
    tx0-8 .. tx0+71 (inside the frame)"""
    H, W = mask.shape
    tiles_x, tiles_y = tile_grid(H, W)
    out = np.zeros((tiles_y, tiles_x), bool)
    for ty in range(tiles_y):
        rows = np.unique(reflect(np.arange(ty * TH - halo, ty * TH + TH + halo), H))
        band = mask[rows].any(axis=0)
        for tx in range(tiles_x):
            out[ty, tx] = band[max(0, tx * TW - 8):min(W, tx * TW + TW + 8)].any()
    return out
