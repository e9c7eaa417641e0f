"""Plain-NumPy restatement of GraspPointSelector.detect_midrib (scripts/utils/grasp_point_selector.py:829-922) and of the
OpenCV pieces it calls: cvtColor(BGR2GRAY) on 8-bit data and CLAHE (clahe.cpp).  float32 where OpenCV computes in float32,
float64 / Python ints where the reference does.  cv2 is not available to pin these against: the formulas are restated from
OpenCV's sources."""
import numpy as np


def bgr2gray(img, mask=None):
    """8-bit BGR2GRAY by channel index; pixels off `mask` are 0 (cv2.bitwise_and(raw, raw, mask=mask), :834)."""
    c = img[..., :3].astype(np.int32)
    g = ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)
    if mask is not None:
        g = np.where(np.asarray(mask) != 0, g, np.uint8(0))
    return g


def clahe_tile_size(H, W, tiles_x, tiles_y):
    """(tile width, tile height): padding (BORDER_REFLECT_101 at the end of BOTH dimensions) unless both divide."""
    if W % tiles_x == 0 and H % tiles_y == 0:
        return W // tiles_x, H // tiles_y
    return (W + tiles_x - W % tiles_x) // tiles_x, (H + tiles_y - H % tiles_y) // tiles_y


def _reflect101(p, n):
    q = np.mod(p, 2 * (n - 1))
    return np.where(q < n, q, 2 * (n - 1) - q)


def clahe_luts(gray, clip_limit=3.0, tiles=(8, 8)):
    """Per-tile LUTs [tiles_y][tiles_x][256] uint8 of CLAHE_CalcLut_Body."""
    H, W = gray.shape
    tx, ty = tiles
    tw, th = clahe_tile_size(H, W, tx, ty)
    ys = _reflect101(np.arange(th * ty), H)
    xs = _reflect101(np.arange(tw * tx), W)
    ext = gray[np.ix_(ys, xs)]
    area = tw * th
    clip = 0
    if clip_limit > 0.0:
        clip = max(int(clip_limit * area / 256), 1)
    scale = np.float32(255.0) / np.float32(area)
    luts = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(hist - clip, 0).sum())
                hist = np.minimum(hist, clip)
                batch, residual = divmod(clipped, 256)
                hist += batch
                if residual:
                    step = max(256 // residual, 1)
                    k = 0
                    while k < 256 and residual > 0:
                        hist[k] += 1
                        k += step
                        residual -= 1
            v = np.cumsum(hist).astype(np.float32) * scale
            luts[j, i] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return luts


def clahe(gray, clip_limit=3.0, tiles=(8, 8)):
    """cv2.createCLAHE(clip_limit, tiles).apply(gray): float32 bilinear interpolation of the tile LUTs, half-even rounding."""
    gray = np.asarray(gray, np.uint8)
    H, W = gray.shape
    tx, ty = tiles
    tw, th = clahe_tile_size(H, W, tx, ty)
    luts = clahe_luts(gray, clip_limit, tiles)
    f32 = np.float32
    txf = np.arange(W, dtype=np.float32) * (f32(1.0) / f32(tw)) - f32(0.5)
    tx1 = np.floor(txf).astype(np.int64)
    xa = txf - tx1.astype(np.float32)
    xa1 = f32(1.0) - xa
    tx2 = np.minimum(tx1 + 1, tx - 1)
    tx1 = np.maximum(tx1, 0)
    tyf = np.arange(H, dtype=np.float32) * (f32(1.0) / f32(th)) - f32(0.5)
    ty1 = np.floor(tyf).astype(np.int64)
    ya = (tyf - ty1.astype(np.float32))[:, None]
    ya1 = f32(1.0) - ya
    ty2 = np.minimum(ty1 + 1, ty - 1)
    ty1 = np.maximum(ty1, 0)
    v = gray.astype(np.int64)
    Y1, Y2 = ty1[:, None], ty2[:, None]
    X1, X2 = tx1[None, :], tx2[None, :]
    l11 = luts[Y1, X1, v].astype(np.float32)
    l12 = luts[Y1, X2, v].astype(np.float32)
    l21 = luts[Y2, X1, v].astype(np.float32)
    l22 = luts[Y2, X2, v].astype(np.float32)
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def midrib_walk(enhanced, mask, orientation):
    """Steps 4-7 of detect_midrib (:858-922) on a given enhanced image.  orientation: (angle, major, minor, (cx, cy)) with
    angle None for no contour.  Returns (status, result): status 0 found, 1 no contour, 2 int(minor / 6) == 0 (cv2.line
    raises), 3 fewer than two points; result ((x0, y0), (x1, y1)) of Python ints or None."""
    angle, major_axis, minor_axis, center = orientation
    if angle is None:
        return 1, None
    center = (int(center[0]), int(center[1]))
    dx = int(major_axis / 2 * np.cos(angle))
    dy = int(major_axis / 2 * np.sin(angle))
    mask_width = int(minor_axis / 6)
    if mask_width <= 0:
        return 2, None
    window_width = mask_width
    H, W = mask.shape
    pts = []
    for t in np.linspace(0, 1, 20):
        x = int(center[0] - dx + 2 * dx * t)
        y = int(center[1] - dy + 2 * dy * t)
        if 0 <= x < W and 0 <= y < H:
            perp_dx = -dy / np.sqrt(dx * dx + dy * dy) * window_width
            perp_dy = dx / np.sqrt(dx * dx + dy * dy) * window_width
            intensities, positions = [], []
            for s in np.linspace(-1, 1, window_width):
                sx = int(x + s * perp_dx)
                sy = int(y + s * perp_dy)
                if 0 <= sx < W and 0 <= sy < H and mask[sy, sx]:
                    intensities.append(enhanced[sy, sx])
                    positions.append((sx, sy))
            if intensities:
                pts.append(positions[int(np.argmax(intensities))])
    if len(pts) < 2:
        return 3, None
    return 0, (tuple(map(int, pts[0])), tuple(map(int, pts[-1])))


def detect_midrib(mask, image, orientation):
    """The whole method: masked gray, CLAHE(3.0, (8, 8)) of the frame, walk with the given orientation."""
    enhanced = clahe(bgr2gray(image, mask), 3.0, (8, 8))
    return midrib_walk(enhanced, mask, orientation)
