"""Independent reference of the inference CNN's weight buffers: what lg_cnn_load / lg_cnn_load_from_trainer leave on the device
for a GraspPointCNN state dict, in numpy float64 rounded once to float32.

Written from the layout comments of csrc/lg_cnn.h and csrc/lg_cnn_load.hip, with elementwise numpy operations in the fold
kernels' association order (numpy does not contract a * b + c into an FMA, and neither do the kernels):
  scale        g / sqrt(v + eps), eps the float32 value promoted
  bconv        (b - mean) * scale + beta                                   [coutp], padded channels 0
  wconv        w * scale                                                   [tap][cinp][coutp]
  uwino        G2 (w * scale) G2^T, rows 0.5 * (a + b + c), a - b + c      F(2x2,3x3), position 4 i + j
  uwino4       G4 (w * scale) G4^T, left-to-right sums of three products   F(4x4,3x3), position 6 i + j
  fcw, fcb     w * sc transposed to [in][out]; b * sc + (beta - mean * sc); the last layer with sc = 1, shift 0
Fragment orders (lane = (ci % 4) * 16 + co % 16):
  uwino        [ci / 4][co / 16][position / 4][lane][position % 4]
  uwino4       [ci / 4][co / 64][(co % 64) / 16][position / 4][lane][position % 4]; layer 0 has 12 input planes
The packers below index element by element; the un-packers reshape and transpose, so one checks the other
(tests/test_cnn_fold_ref.py)."""
import numpy as np

EPS = np.float32(1e-5)   # lg_cnn_weights.bn_eps as cnn.pack_state_dict sets it: a float

G2 = np.array([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]])
G4 = np.array([[1.0 / 4, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6],
               [1.0 / 24, 1.0 / 12, 1.0 / 6], [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1.0]])


def pad64(c):
    return (c + 63) // 64 * 64


def layer_plan(filters):
    """[(cin, cout, cinp, coutp)] of the encoder: two convs per block, channels padded to 64 (the 9 input planes to 10)."""
    out, cin, cinp = [], 9, 10
    for f in filters:
        out += [(cin, f, cinp, pad64(f)), (f, f, pad64(f), pad64(f))]
        cin, cinp = f, pad64(f)
    return out


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def bn_scale(g, v, eps=EPS):
    return _f64(g) / np.sqrt(_f64(v) + np.float64(np.float32(eps)))


def fold_conv(w, b, g, beta, mean, var, eps=EPS):
    """-> (folded weights [co][ci][3][3], folded bias [co]), float64, not rounded."""
    sc = bn_scale(g, var, eps)
    return _f64(w) * sc[:, None, None, None], (_f64(b) - _f64(mean)) * sc + _f64(beta)


def fold_fc(w, b, g=None, beta=None, mean=None, var=None, eps=EPS):
    """-> (weights [out][in], bias [out]), float64, not rounded; g = None: a layer without BatchNorm1d."""
    n = np.asarray(b).shape[0]
    sc, sh = np.ones(n), np.zeros(n)
    if g is not None:
        sc = bn_scale(g, var, eps)
        sh = _f64(beta) - _f64(mean) * sc
    return _f64(w) * sc[:, None], _f64(b) * sc + sh


def wino2(wf):
    """F(2x2,3x3) U = G g G^T of folded weights [co][ci][3][3] -> [co][ci][4][4], in the kernels' order of operations."""
    g0, g1, g2 = wf[:, :, 0, :], wf[:, :, 1, :], wf[:, :, 2, :]
    gg = np.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2], axis=2)       # [co][ci][4][3]
    c0, c1, c2 = gg[..., 0], gg[..., 1], gg[..., 2]
    return np.stack([c0, 0.5 * (c0 + c1 + c2), 0.5 * (c0 - c1 + c2), c2], axis=3)


def wino4(wf):
    """F(4x4,3x3) U = G g G^T -> [co][ci][6][6]: every entry G[i][0] * a + G[i][1] * b + G[i][2] * c, zeros included."""
    gg = np.stack([G4[i, 0] * wf[:, :, 0, :] + G4[i, 1] * wf[:, :, 1, :] + G4[i, 2] * wf[:, :, 2, :] for i in range(6)], axis=2)
    return np.stack([gg[..., 0] * G4[j, 0] + gg[..., 1] * G4[j, 1] + gg[..., 2] * G4[j, 2] for j in range(6)], axis=3)


def _grid(cout, cin, npos):
    return np.meshgrid(np.arange(cout), np.arange(cin), np.arange(npos), indexing="ij")


def pack_direct(wf, cinp, coutp):
    """[co][ci][3][3] -> flat [tap][cinp][coutp]."""
    cout, cin = wf.shape[:2]
    co, ci, tap = _grid(cout, cin, 9)
    out = np.zeros(9 * cinp * coutp, wf.dtype)
    out[(tap * cinp + ci) * coutp + co] = wf.reshape(cout, cin, 9)
    return out


def pack_wino2(u, cinp, coutp):
    """[co][ci][4][4] -> flat fragment order of lg_wino_kernel."""
    cout, cin = u.shape[:2]
    co, ci, pos = _grid(cout, cin, 16)
    out = np.zeros(16 * cinp * coutp, u.dtype)
    out[((((ci // 4) * (coutp // 16) + co // 16) * 4 + pos // 4) * 64 + (ci % 4) * 16 + co % 16) * 4 + pos % 4] = u.reshape(cout, cin, 16)
    return out


def pack_wino4(u, cinp4, coutp):
    """[co][ci][6][6] -> flat fragment order of lg_wino4_kernel."""
    cout, cin = u.shape[:2]
    co, ci, pos = _grid(cout, cin, 36)
    out = np.zeros(36 * cinp4 * coutp, u.dtype)
    out[(((((ci // 4) * (coutp // 64) + co // 64) * 4 + (co % 64) // 16) * 9 + pos // 4) * 64 + (ci % 4) * 16 + co % 16) * 4
        + pos % 4] = u.reshape(cout, cin, 36)
    return out


def unpack_direct(flat, cinp, coutp):
    """-> [coutp][cinp][9]"""
    return flat.reshape(9, cinp, coutp).transpose(2, 1, 0)


def unpack_wino2(flat, cinp, coutp):
    """-> [coutp][cinp][16]"""
    a = flat.reshape(cinp // 4, coutp // 16, 4, 4, 16, 4)          # ci/4, co/16, q, ci%4, co%16, pos%4
    return a.transpose(1, 4, 0, 3, 2, 5).reshape(coutp, cinp, 16)


def unpack_wino4(flat, cinp4, coutp):
    """-> [coutp][cinp4][36]"""
    a = flat.reshape(cinp4 // 4, coutp // 64, 4, 9, 4, 16, 4)      # ci/4, co/64, cb, pg, ci%4, co%16, pos%4
    return a.transpose(1, 2, 5, 0, 4, 3, 6).reshape(coutp, cinp4, 36)


def encoder_filters_of(state):
    f = []
    while f"encoder.{len(f)}.0.weight" in state:
        f.append(int(np.asarray(state[f"encoder.{len(f)}.0.weight"]).shape[0]))
    return tuple(f)


def fold_reference(state, eps=EPS):
    """{(name, layer): flat float32 array} for bconv, wconv, uwino, uwino4 (encoder layers) and fcw, fcb (classifier layers);
    no entry where the model has no such buffer (uwino of layer 0, wconv past layer 0 of a non-standard encoder)."""
    filters = encoder_filters_of(state)
    standard = filters == (64, 128, 256)
    out = {}
    for L, (cin, cout, cinp, coutp) in enumerate(layer_plan(filters)):
        conv, bn = f"encoder.{L // 2}.{(0, 3)[L % 2]}", f"encoder.{L // 2}.{(1, 4)[L % 2]}"
        wf, bf = fold_conv(state[conv + ".weight"], state[conv + ".bias"], state[bn + ".weight"], state[bn + ".bias"],
                           state[bn + ".running_mean"], state[bn + ".running_var"], eps)
        out["bconv", L] = np.concatenate([bf, np.zeros(coutp - cout)]).astype(np.float32)
        if L == 0 or standard:
            out["wconv", L] = pack_direct(wf, cinp, coutp).astype(np.float32)
        if L >= 1:
            out["uwino", L] = pack_wino2(wino2(wf), cinp, coutp).astype(np.float32)
        out["uwino4", L] = pack_wino4(wino4(wf), 12 if L == 0 else cinp, coutp).astype(np.float32)
    for L, idx in enumerate((0, 4, 8, 12)):
        fc, bn = f"classifier.{idx}", f"classifier.{idx + 1}"
        args = [state[bn + ".weight"], state[bn + ".bias"], state[bn + ".running_mean"], state[bn + ".running_var"]] if L < 3 else []
        wt, bt = fold_fc(state[fc + ".weight"], state[fc + ".bias"], *args, eps=eps)
        out["fcw", L] = np.ascontiguousarray(wt.T).reshape(-1).astype(np.float32)
        out["fcb", L] = bt.astype(np.float32)
    return out
