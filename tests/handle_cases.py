"""Scenes, a step vocabulary and stream cases for the tests that keep ONE handle across calls (tests/test_gpu_call_sequences.py,
tests/test_gpu_stream_order.py; the conditions that make them able to fail: tests/test_handle_cases_host.py).  No tests here.

  scenes     label images of a few ellipses (label_aware_ref.blob_labels) at 96 x 320 ("wide": 6 x 5 tiles of 64 x 16) and
             160 x 192 ("tall"), leaf 1 the current leaf, with an empty, a full-frame and a speckled frame (more runs than a
             small LG_ORIENT_CAP holds).  A, B, C have distinct picks, D has no valid pixel (its pick moves with the CNN).
  steps      (entry, set, scenes, options) -> run_step(handle, step): a canonical byte string of everything the call returns.
             expected(step, model, env): the same step on a handle created for it alone, memoised.
  streams    run_stream_case(): delay, copy of the true scene into the persistent inputs, the library call, in-stream clones of
             its outputs, copy of the decoy back -- all on one caller stream without a host wait.  `python -m tests.handle_cases
             --streams` runs every case in a process of its own and prints one JSON line per case."""
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import label_aware_ref as R  # noqa: E402
from tests import midrib_scenes  # noqa: E402

# ----------------------------------------------------------------------------------------------------------------- scenes
# (id, cx, cy, rx, ry); leaf 1 is the current leaf of every scene
SETS = {
    "wide": dict(H=96, W=320, scenes={
        "A": [(1, 60, 40, 34, 26), (2, 110, 40, 8, 10)],
        "B": [(1, 250, 52, 36, 28), (2, 200, 20, 10, 8)],
        "C": [(1, 160, 48, 50, 30)],
        "D": [(1, 30, 70, 28, 22), (2, 300, 10, 12, 8)],
    }),
    "tall": dict(H=160, W=192, scenes={
        "A": [(1, 60, 45, 34, 28), (2, 106, 45, 6, 10)],
        "B": [(1, 163, 56, 27, 46), (2, 128, 100, 6, 8)],
        "C": [(1, 96, 60, 60, 36)],
        "D": [(1, 150, 135, 30, 22), (2, 30, 12, 12, 8)],
    }),
}
LETTERS = ("A", "B", "C", "D")
ORDER = ("A", "B", "C", "D", "empty", "full", "over")
ORIENT_CAP = 64   # the small run scratch of sequence 7: "over" has more runs, A has fewer


def shape_of(set_):
    return SETS[set_]["H"], SETS[set_]["W"]


def P_of(set_):
    H, W = shape_of(set_)
    P = np.zeros((3, 4))
    P[0, 0] = P[1, 1] = 600.0
    P[0, 2], P[1, 2], P[0, 3] = W / 2.0, H / 2.0, -60.0
    return P


def depth_of(H, W, phase=0.0, z=0.45):
    yy, xx = np.mgrid[:H, :W]
    return (z + 0.002 * np.sin(xx / 7.0 + phase) + 0.002 * np.cos(yy / 5.0 - phase)).astype(np.float32)


_scene_memo = {}


def scene(set_, name):
    """(labels int16 [H, W], depth float32 [H, W]); read-only arrays, computed once"""
    key = (set_, name)
    if key not in _scene_memo:
        H, W = shape_of(set_)
        if name in LETTERS:
            lab = R.blob_labels(H, W, SETS[set_]["scenes"][name])
        elif name == "empty":
            lab = np.zeros((H, W), np.int16)
        elif name == "full":
            lab = np.ones((H, W), np.int16)
        elif name == "over":   # leaf A and specks of the same label: one run each
            lab = R.blob_labels(H, W, SETS[set_]["scenes"]["A"][:1])
            lab[np.random.default_rng(11).random((H, W)) > 0.985] = 1
        else:
            raise KeyError(name)
        dep = depth_of(H, W, phase=0.7 * ORDER.index(name), z=0.45 + 0.01 * ORDER.index(name))
        lab.setflags(write=False)
        dep.setflags(write=False)
        _scene_memo[key] = (lab, dep)
    return _scene_memo[key]


def batch(set_, names):
    labs, deps = zip(*(scene(set_, n) for n in names))
    return np.stack(labs), np.stack(deps)


def runs_of(mask):
    """horizontal runs of a 2-D mask: what the orientation kernel's scratch counts"""
    m = np.pad(np.asarray(mask, np.int8), ((0, 0), (1, 0)))
    return int((np.diff(m, axis=1) == 1).sum())


# ------------------------------------------------------------------------------------------------------------------ steps
def S(entry, set_="wide", scenes=(), **opts):
    return (entry, set_, tuple(scenes), tuple(sorted(opts.items())))


ENTRIES = ("select", "score_maps", "leaves", "cands", "cands_leaves", "set_cnn", "clear_cnn", "load_trainer", "cnn_forward",
           "evaluate", "topk", "gather", "orient", "midrib", "negmasks", "harvest", "refused")
MODEL_STEPS = ("set_cnn", "clear_cnn", "load_trainer")
SPLIT_N = 20   # lg_cnn_forward at 20 patches splits the left-over items of its 256-channel layers (launch_wino4_rt)


def vocabulary(set_):
    """every step the random walk draws from, at one shape"""
    v = []
    for sc in (("A",), ("B",), ("C",), ("D",), ("empty",), ("full",), ("over",)):
        v += [S("select", set_, sc), S("select", set_, sc, dense=1)]
    v += [S("select", set_, ("A",), bool=1), S("select", set_, ("D",), bool=1), S("select", set_, ("B",), g=1),
          S("select", set_, ("B",), g=7), S("select", set_, ("A", "empty", "C"), dense=1), S("select", set_, ("A", "B", "C")),
          S("select", set_, ("C", "empty", "A", "D", "B", "full", "A")), S("score_maps", set_, ("A",)),
          S("score_maps", set_, ("C", "B")), S("score_maps", set_, ("B",), g=7)]
    for la in (0, 1):
        v += [S("leaves", set_, ("A",), la=la), S("leaves", set_, ("B", "C", "A"), la=la), S("leaves", set_, ("A",), la=la, id=7),
              S("cands_leaves", set_, ("A",), la=la), S("cands_leaves", set_, ("B", "D"), la=la, k=1)]
    for k in (1, 20, 64):
        v += [S("cands", set_, ("A",), k=k), S("cands", set_, ("D", "B", "C"), k=k)]
    v += [S("set_cnn", set_, seed=0), S("set_cnn", set_, seed=1), S("clear_cnn", set_), S("load_trainer", set_, seed=0),
          S("load_trainer", set_, seed=1), S("cnn_forward", set_, n=SPLIT_N), S("cnn_forward", set_, n=1), S("evaluate", set_),
          S("topk", set_, ("B",)), S("topk", set_, ("C",)), S("gather", set_, ("C",)), S("orient", set_), S("midrib", set_),
          S("negmasks", set_, ("B",)), S("harvest", set_, ("C",)), S("refused", set_, ("A",), kind="g9"),
          S("refused", set_, ("A",), kind="la_mask"), S("refused", set_, ("A",), kind="pcl")]
    return v


def _torch():
    import torch
    return torch


def _b(*parts):
    torch = _torch()
    out = []
    for p in parts:
        if torch.is_tensor(p):
            p = p.detach().cpu().numpy()
        if isinstance(p, np.ndarray):
            out.append(np.ascontiguousarray(p).tobytes())
        elif isinstance(p, (bytes, bytearray)):
            out.append(bytes(p))
        else:
            out.append(repr(p).encode())
    return b"|".join(out)


class _Env:
    """the options a handle reads at lg_create (all of them, LG_ORIENT_CAP too: lg_debug_options), set for the time of the creation
    and of every step on the handle, and put back"""

    def __init__(self, env):
        self.env = dict(env or ())

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update({k: str(v) for k, v in self.env.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_cnn_memo = {}


def cnn_params(seed):
    from oracle import lg_oracle as O
    if seed not in _cnn_memo:
        _cnn_memo[seed] = O.cnn_closed_form_params(seed=seed)
    return _cnn_memo[seed]


_trainers = {}


def trainer_holding(seed):
    torch = _torch()
    from leafgrasp_amd.trainer import GraspTrainer
    if seed not in _trainers:
        tr = GraspTrainer(torch.device("cuda:0"), max_batch=4)
        tr.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cnn_params(seed).items()})
        _trainers[seed] = tr
    return _trainers[seed]


class Handle:
    """one GraspPointSelector and what the steps have done to its model; env: options read at lg_create"""

    def __init__(self, set_="wide", env=(), model="none"):
        torch = _torch()
        import leafgrasp_amd as L
        self.env = tuple(sorted(dict(env).items()))
        with _Env(self.env):
            self.sel = L.GraspPointSelector(torch.device("cuda:0"), load_model=False)
        self.sel.set_camera_params(P_of(set_))
        self.set = set_
        self.model = "none"
        if model != "none":
            run_step(self, S("set_cnn", set_, seed=int(model[-1])))


_ips = {}


def _ip(set_, g):
    import leafgrasp_amd as L
    if (set_, g) not in _ips:
        H, W = shape_of(set_)
        _ips[(set_, g)] = L.ImageProcessor(H, W, 21, g)
    return _ips[(set_, g)]


_planes = {}


def planes_of(set_, name):
    """the eight planes and the validity plane of a scene (numpy), from a handle of their own: inputs of the foreign entries"""
    from leafgrasp_amd._lib import MAP_NAMES
    torch = _torch()
    if (set_, name) not in _planes:
        lab, dep = scene(set_, name)
        hd = Handle(set_)
        maps, valid, _ = hd.sel.score_maps(torch.from_numpy((lab == 1).astype(np.uint8)).cuda(), torch.from_numpy(dep).cuda())
        torch.cuda.synchronize()
        out = {n: maps[n].cpu().numpy() for n in MAP_NAMES}
        out["valid"] = valid.cpu().numpy()
        _planes[(set_, name)] = out
    return _planes[(set_, name)]


def points_of(set_):
    H, W = shape_of(set_)
    return [(40, 40), (16, 16), (W - 16, H - 16), (W // 2, H // 2), (W - 20, 30), (5, 5), (W - 1, H - 1), (70, 50)]


def orient_mask():
    yy, xx = np.mgrid[0:300, 0:200]
    return ((((xx - 100 - 0.25 * (yy - 150)) / 60.0) ** 2 + ((yy - 150) / 120.0) ** 2) <= 1.0).astype(np.uint8)


def patches_of(n, seed=5):
    from oracle import lg_oracle as O
    return np.ascontiguousarray(O.synthetic_patches(n, seed=seed), np.float32)


def _map_ptrs(tensors):
    from leafgrasp_amd._lib import LG_NUM_MAPS
    ptrs = (C.c_void_p * LG_NUM_MAPS)()
    for i, t in enumerate(tensors):
        ptrs[i] = t.data_ptr()
    return ptrs


def run_step(hd, step):
    """the step on this handle -> canonical bytes of everything it returns.  A call the library refuses gives b'refused'."""
    from leafgrasp_amd import _lib
    try:
        with _Env(hd.env):
            return _run_step(hd, step)
    except _lib.LgError as e:
        return b"refused: " + str(e).split(":")[0].encode()


def _run_step(hd, step):
    torch = _torch()
    from leafgrasp_amd import _lib
    from leafgrasp_amd._lib import MAP_NAMES, lib
    entry, set_, names, opts = step
    o = dict(opts)
    sel = hd.sel
    H, W = shape_of(set_)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    if names:
        lab, dep = batch(set_, names)
        m = lab == 1
    if entry == "select":
        mt, dt = cuda(m if o.get("bool") else m.astype(np.uint8)), cuda(dep)
        ip = _ip(set_, o.get("g", 5))
        if o.get("dense"):
            _, maps, valid = sel.select_grasp_points_batch(mt, dt, return_maps=True, image_processor=ip)
            return _b(bytes(sel.last_results), *[maps[n] for n in MAP_NAMES], valid)
        sel.select_grasp_points_batch(mt, dt, image_processor=ip)
        return _b(bytes(sel.last_results))
    if entry == "score_maps":
        maps, valid, theta = sel.score_maps(cuda(m.astype(np.uint8)), cuda(dep), _ip(set_, o.get("g", 5)))
        return _b(*[maps[n] for n in MAP_NAMES], valid, theta)
    if entry in ("leaves", "cands_leaves"):
        ids = [o.get("id", 1)] * len(names)
        if entry == "leaves":
            sel.select_grasp_points_for_leaves(cuda(lab), ids, cuda(dep), label_aware=bool(o["la"]))
            return _b(bytes(sel.last_results))
        _, c = sel.select_grasp_candidates_for_leaves(cuda(lab), ids, cuda(dep), top_k=o.get("k", 20), label_aware=bool(o["la"]))
        return _b(bytes(sel.last_results), c.tobytes())
    if entry == "cands":
        _, c = sel.select_grasp_candidates_batch(cuda(m.astype(np.uint8)), cuda(dep), top_k=o.get("k", 20))
        return _b(bytes(sel.last_results), c.tobytes())
    if entry == "set_cnn":
        sel.set_cnn_state_dict(cnn_params(o["seed"]))
        hd.model = f"seed{o['seed']}"
        return b""
    if entry == "clear_cnn":
        sel.clear_cnn()
        hd.model = "none"
        return b""
    if entry == "load_trainer":
        sel.load_from_trainer(trainer_holding(o["seed"]))
        hd.model = f"seed{o['seed']}"
        return b""
    if entry == "cnn_forward":
        return _b(sel.cnn_forward(cuda(patches_of(o["n"]))))
    if entry == "evaluate":
        n = 37
        r = sel.evaluate(cuda(patches_of(n, seed=9)), cuda((np.arange(n) % 3 == 0).astype(np.float32)), return_logits=True)
        return _b((r["val_loss"], r["accuracy"], r["n"], sorted(r["metrics"].items())), r["logits"])
    if entry == "topk":
        pl = planes_of(set_, names[0])
        got = sel._get_candidate_points(pl["traditional_score"], pl["valid"], top_k=o.get("k", 20))
        assert got, "the mirror swallows errors and returns []: this scene has candidates"
        return _b(got)
    if entry == "gather":
        pl = planes_of(set_, names[0])
        return _b(sel.gather_patches(cuda(m[0].astype(np.uint8)), cuda(dep[0]), {n: pl[n] for n in MAP_NAMES}, points_of(set_)[:4]))
    if entry == "orient":
        return _b(sel.estimate_leaf_orientation(orient_mask()))
    if entry == "midrib":
        mk, img = midrib_scenes.leaf_scene(H, W, np.random.default_rng(4))
        return _b(sel.detect_midrib(mk, img), getattr(sel, "last_midrib_status", None))
    if entry == "negmasks":
        pl = planes_of(set_, names[0])
        d, mt = cuda(pl["distance_map"]), cuda(m[0].astype(np.uint8))
        tip, stem = torch.full((H, W), 7, dtype=torch.uint8, device="cuda"), torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
        _lib.check(sel._h, lib.lg_negative_masks(sel._h, d.data_ptr(), mt.data_ptr(), H, W, tip.data_ptr(), stem.data_ptr(),
                                                 sel._stream()), "lg_negative_masks")
        torch.cuda.synchronize()
        return _b(tip, stem)
    if entry == "harvest":
        pl = planes_of(set_, names[0])
        pts = points_of(set_)
        n = len(pts)
        d, mt = cuda(dep[0]), cuda(m[0].astype(np.uint8))
        planes = [cuda(pl[k]) for k in MAP_NAMES[:7]]
        xy = torch.tensor(pts, dtype=torch.int32, device="cuda").contiguous()
        rot = torch.arange(n, dtype=torch.int32, device="cuda")
        od, om = torch.full((n, 32, 32), -7.0, device="cuda"), torch.full((n, 32, 32), -7.0, device="cuda")
        osc, fl = torch.full((n, 7, 32, 32), -7.0, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda")
        ptrs = _map_ptrs(planes)
        _lib.check(sel._h, lib.lg_harvest_patches(sel._h, d.data_ptr(), mt.data_ptr(), C.byref(ptrs), H, W, n, xy.data_ptr(),
                                                  rot.data_ptr(), od.data_ptr(), om.data_ptr(), osc.data_ptr(), fl.data_ptr(),
                                                  sel._stream()), "lg_harvest_patches")
        torch.cuda.synchronize()
        return _b(od, om, osc, fl)
    if entry == "refused":
        mt, dt = cuda(m.astype(np.uint8)), cuda(dep)
        if o["kind"] == "pcl":   # the reference raises in its point-cloud branch: the logged None triple
            got = sel.select_grasp_point(mt[0], dt[0], pcl_data=object())
            assert got == (None, None, None)
            return _b(got)
        p = _lib.LgParams.from_buffer_copy(sel._sync_params(None))
        if o["kind"] == "g9":
            p.gaussian_size = 9
        else:
            p.label_aware = 1
        res = (_lib.LgGraspResult * len(names))()
        rc = lib.lg_select_grasp(sel._h, dt.data_ptr(), mt.data_ptr(), len(names), H, W, C.byref(p), None, None, res, sel._stream())
        assert rc in (_lib.LG_ERR_INVALID, _lib.LG_ERR_UNSUPPORTED), rc
        return _b("refused", rc)
    raise KeyError(entry)


_expected = {}


def expected(step, model="none", env=()):
    """the step on a handle created for it alone (with the model and the options of the handle under test), memoised"""
    key = (step, model if step[0] not in MODEL_STEPS else "", tuple(sorted(dict(env).items())))
    if key not in _expected:
        _expected[key] = run_step(Handle(step[1], env, model), step)
    return _expected[key]


def walk(hd, steps, note=""):
    """every step on one handle, each held to its fresh-handle bytes; returns the bytes"""
    out, hist = [], []
    for i, st in enumerate(steps):
        model = hd.model
        got, want = run_step(hd, st), expected(st, model, hd.env)
        assert got == want, f"{note}step {i} {st} (model {model}) differs from a fresh handle; the steps before it: {hist[-3:]}"
        hist.append(st)
        out.append(got)
    return out


# ---------------------------------------------------------------------------------------------------------- stream cases
class Built:
    """ins: persistent device tensors; true / decoy: the numpy arrays copied into them; call() -> (host values, out tensors)"""

    def __init__(self, ins, true, decoy, call, keep=(), warm=None):
        self.ins, self.true, self.decoy, self.call, self.keep = ins, true, decoy, call, keep
        self.warm = warm or call   # what builds the workspace before the timed run; must leave the answer of call() alone
        self.env = getattr(keep[0], "env", ()) if keep else ()


def _select_case(mode, true, decoy, env=(), set_="wide", cnn=0):
    def build():
        torch = _torch()
        hd = Handle(set_, env, f"seed{cnn}" if cnn is not None else "none")
        sel = hd.sel
        (tl, td), (dl, dd) = batch(set_, true), batch(set_, decoy)
        if mode in ("labels", "cands_labels"):
            tin, din = [tl, td], [dl, dd]
        else:
            tin, din = [(tl == 1).astype(np.uint8), td], [(dl == 1).astype(np.uint8), dd]
        ins = [torch.from_numpy(a.copy()).cuda() for a in din]
        ids = [1] * len(true)

        def call():
            if mode == "sparse":
                sel.select_grasp_points_batch(ins[0], ins[1])
                return [bytes(sel.last_results)], []
            if mode == "dense":
                _, maps, valid = sel.select_grasp_points_batch(ins[0], ins[1], return_maps=True)
                return [bytes(sel.last_results)], list(maps.values()) + [valid]
            if mode == "labels":
                sel.select_grasp_points_for_leaves(ins[0], ids, ins[1], label_aware=True)
                return [bytes(sel.last_results)], []
            _, c = sel.select_grasp_candidates_batch(ins[0], ins[1])
            return [bytes(sel.last_results), c.tobytes()], []
        return Built(ins, tin, din, call, keep=(hd,))
    return build


def _maps_case(twice):
    def build():
        torch = _torch()
        from leafgrasp_amd import _lib
        hd = Handle("wide")
        sel, (H, W) = hd.sel, shape_of("wide")
        true, decoy, ins, outs = [], [], [], []
        for t, d in ((("A", "B"), ("C", "B")) if twice else (("A", "B"),)):
            (tl, td), (dl, dd) = scene("wide", t), scene("wide", d)
            true += [(tl == 1).astype(np.uint8)[None], td[None]]
            decoy += [(dl == 1).astype(np.uint8)[None], dd[None]]
            outs.append((torch.zeros((8, 1, H, W), device="cuda"), torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")))
        ins = [torch.from_numpy(a.copy()).cuda() for a in decoy]
        p = _lib.LgParams.from_buffer_copy(sel._sync_params(None))

        def call():
            thetas = []
            for i, (maps, valid) in enumerate(outs):
                th = (C.c_float * 1)()
                ptrs = _map_ptrs([maps[j] for j in range(8)])
                _lib.check(sel._h, _lib.lib.lg_score_maps(sel._h, ins[2 * i + 1].data_ptr(), ins[2 * i].data_ptr(), 1, H, W, C.byref(p),
                                                          C.byref(ptrs), valid.data_ptr(), th, sel._stream()), "lg_score_maps")
                thetas.append(bytes(th))
            return thetas, [t for pair in outs for t in pair]
        return Built(ins, true, decoy, call, keep=(hd,))
    return build


def _plain_case(kind):
    """the entries that take planes or images and enqueue on the caller's stream"""
    def build():
        torch = _torch()
        from leafgrasp_amd import _lib
        from leafgrasp_amd._lib import MAP_NAMES, lib
        hd = Handle("wide", model="seed0" if kind == "cnn_forward" else "none")
        sel, (H, W) = hd.sel, shape_of("wide")
        h = sel._h
        st = sel._stream

        def planes(name):
            pl, (lab, dep) = planes_of("wide", name), scene("wide", name)
            return [dep, (lab == 1).astype(np.uint8), np.stack([pl[n] for n in MAP_NAMES]), pl["valid"]]
        if kind == "smooth":
            true, decoy = [scene("wide", "A")[1][None]], [scene("wide", "B")[1][None]]
        elif kind in ("topk", "gather", "harvest", "negmasks"):
            true, decoy = planes("A"), planes("B")
        elif kind == "cnn_forward":
            true, decoy = [patches_of(SPLIT_N, 5)], [patches_of(SPLIT_N, 6)]
        elif kind == "clahe":
            rng = np.random.default_rng(3)
            true, decoy = [rng.integers(0, 255, (1, H, W), dtype=np.uint8)], [rng.integers(40, 200, (1, H, W), dtype=np.uint8)]
        elif kind in ("midrib", "orient"):
            (mt, it), (md, idc) = (midrib_scenes.leaf_scene(H, W, np.random.default_rng(s)) for s in (4, 5))
            true, decoy = ([it[None], mt[None]], [idc[None], md[None]]) if kind == "midrib" else ([mt], [md])
        ins = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in decoy]
        pts = points_of("wide")
        xy = torch.tensor(pts, dtype=torch.int32, device="cuda").reshape(1, len(pts), 2).contiguous()
        n = torch.tensor([len(pts)], dtype=torch.int32, device="cuda")
        rot = torch.arange(len(pts), dtype=torch.int32, device="cuda")
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")   # noqa: E731

        def call():
            if kind == "smooth":
                out = z(1, H, W)
                _lib.check(None, lib.lg_smooth_depth(h, ins[0].data_ptr(), 1, H, W, 5, out.data_ptr(), st()), "lg_smooth_depth")
                return [], [out]
            if kind == "topk":
                oxy, on = z(1, 20, 2, dt=torch.int32), z(1, dt=torch.int32)
                _lib.check(h, lib.lg_topk_nms(h, ins[2][7].data_ptr(), ins[3].data_ptr(), 1, H, W, 20, 10, oxy.data_ptr(), on.data_ptr(),
                                              st()), "lg_topk_nms")
                return [], [oxy, on]
            if kind == "gather":
                out = z(1, len(pts), 9, 32, 32)
                ptrs = _map_ptrs([ins[2][j] for j in range(8)])
                _lib.check(h, lib.lg_gather_patches(h, ins[0].data_ptr(), ins[1].data_ptr(), C.byref(ptrs), 1, H, W, len(pts),
                                                    xy.data_ptr(), n.data_ptr(), out.data_ptr(), st()), "lg_gather_patches")
                return [], [out]
            if kind == "harvest":
                od, om, osc, fl = z(len(pts), 32, 32), z(len(pts), 32, 32), z(len(pts), 7, 32, 32), z(len(pts), dt=torch.int32)
                ptrs = _map_ptrs([ins[2][j] for j in range(7)])
                _lib.check(h, lib.lg_harvest_patches(h, ins[0].data_ptr(), ins[1].data_ptr(), C.byref(ptrs), H, W, len(pts),
                                                     xy.data_ptr(), rot.data_ptr(), od.data_ptr(), om.data_ptr(), osc.data_ptr(),
                                                     fl.data_ptr(), st()), "lg_harvest_patches")
                return [], [od, om, osc, fl]
            if kind == "negmasks":
                tip, stem = z(H, W, dt=torch.uint8), z(H, W, dt=torch.uint8)
                _lib.check(h, lib.lg_negative_masks(h, ins[2][4].data_ptr(), ins[1].data_ptr(), H, W, tip.data_ptr(), stem.data_ptr(),
                                                    st()), "lg_negative_masks")
                return [], [tip, stem]
            if kind == "cnn_forward":
                out = z(SPLIT_N)
                _lib.check(h, lib.lg_cnn_forward(h, ins[0].data_ptr(), SPLIT_N, out.data_ptr(), st()), "lg_cnn_forward")
                return [], [out]
            if kind == "clahe":
                out = z(1, H, W, dt=torch.uint8)
                _lib.check(h, lib.lg_clahe(h, ins[0].data_ptr(), 1, H, W, 3.0, 8, 8, out.data_ptr(), st()), "lg_clahe")
                return [], [out]
            if kind == "midrib":
                return [sel.detect_midrib_batch(ins[1], ins[0]), list(sel.last_midrib_status)], []
            out, found = (C.c_float * 5)(), C.c_int(0)
            _lib.check(h, lib.lg_leaf_orientation(h, ins[0].data_ptr(), H, W, out, C.byref(found), st()), "lg_leaf_orientation")
            return [bytes(out), found.value], []
        return Built(ins, true, decoy, call, keep=(hd,))
    return build


def _leaf_case():
    def build():
        torch = _torch()
        import leafgrasp_amd as L
        ls = L.OptimalLeafSelector(torch.device("cuda:0"))
        ls.set_camera_params(P_of("tall"))
        (tl, td), (dl, dd) = batch("tall", ("C", "A", "B")), batch("tall", ("B", "C", "A"))
        ins = [torch.from_numpy(a.copy()).cuda() for a in (dl, dd)]

        def exact(st):   # sum_depth and sum_ray are added with floating-point atomics: their last bits depend on the order
            keys = ("id", "area", "touches_border", "sum_x", "sum_y", "median_depth")
            return [tuple(float(d[k]) for k in keys) for d in st[0]], st[1], st[2]

        def call():
            stats = ls.leaf_statistics(ins[0][0], ins[1][0])
            return [exact(stats), ls.select_optimal_leaves_batch(ins[0], ins[1]),
                    [exact(st) for st in ls.leaf_statistics_batch(ins[0], ins[1])]], []
        return Built(ins, [tl, td], [dl, dd], call, keep=(ls,))
    return build


def _train_case():
    def build():
        torch = _torch()
        from leafgrasp_amd.trainer import GraspTrainer, dropout_layout
        hd = Handle("wide", model="seed1")
        tr = GraspTrainer(torch.device("cuda:0"), max_batch=4)
        tr.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cnn_params(0).items()})
        ones = [np.ones((4, w), np.float32) for w, _ in dropout_layout((64, 128, 256))]
        y = np.array([0, 1, 0, 1], np.float32)
        true, decoy = [patches_of(4, 2), y, patches_of(SPLIT_N, 5)], [patches_of(4, 3), 1 - y, patches_of(SPLIT_N, 6)]
        ins = [torch.from_numpy(a.copy()).cuda() for a in decoy]

        def call():
            loss = tr.train_step(ins[0], ins[1], masks=ones)
            hd.sel.load_from_trainer(tr)
            return [loss], [hd.sel.cnn_forward(ins[2])]
        return Built(ins, true, decoy, call, keep=(hd, tr), warm=lambda: hd.sel.cnn_forward(ins[2]))   # (a step moves the weights)
    return build


def _cycle(names, n):
    return tuple(names[i % len(names)] for i in range(n))


# name -> (proof of a busy stream, builder).  proof: "host" = the call waits for the caller's stream (the host spends the
# delay inside it), "event" = the call returns while an event behind the delay is still pending.  lg_score_maps waits for its
# orientation kernel, which runs behind the caller's stream: "host".  Every case makes one call on the decoy first
# (Built.warm), so that the workspace exists and its allocation (which synchronises the device) is not what orders the case.
STREAM_CASES = {
    "select sparse, CNN pruning": ("host", _select_case("sparse", ("A",), ("B",))),
    "select dense": ("host", _select_case("dense", ("A",), ("B",))),
    "labels entry, label_aware": ("host", _select_case("labels", ("A",), ("B",))),
    "candidates": ("host", _select_case("cands", ("D",), ("B",))),
    "select, LG_DIRECT_HOST=0": ("host", _select_case("sparse", ("A",), ("B",), env={"LG_DIRECT_HOST": 0})),
    "select, LG_HOST_ORIENT=1": ("host", _select_case("sparse", ("A",), ("B",), env={"LG_HOST_ORIENT": 1})),
    "select, LG_ORIENT_CAP=64, overflowing leaf": ("host", _select_case("sparse", ("over",), ("B",), env={"LG_ORIENT_CAP": ORIENT_CAP})),
    "select, LG_SIDE_TAIL=0": ("host", _select_case("sparse", ("A",), ("B",), env={"LG_SIDE_TAIL": 0})),
    "select, LG_SIDE_TAIL=2": ("host", _select_case("sparse", ("A",), ("B",), env={"LG_SIDE_TAIL": 2})),
    "select, LG_SUBBATCH=2, B=5": ("host", _select_case("sparse", ("A", "C", "D", "A", "C"), ("B", "A", "B", "C", "D"),
                                                        env={"LG_SUBBATCH": 2})),
    "select, B=3": ("host", _select_case("sparse", ("A", "C", "D"), ("B", "A", "C"))),
    "select, B=40": ("host", _select_case("sparse", _cycle("ACDB", 40), _cycle("BACD", 40))),
    "score_maps twice": ("host", _maps_case(True)),
    "smooth_depth": ("event", _plain_case("smooth")),
    "topk_nms": ("event", _plain_case("topk")),
    "gather_patches": ("event", _plain_case("gather")),
    "cnn_forward": ("event", _plain_case("cnn_forward")),
    "clahe": ("event", _plain_case("clahe")),
    "detect_midrib": ("host", _plain_case("midrib")),
    "leaf_orientation": ("host", _plain_case("orient")),
    "leaf stage": ("host", _leaf_case()),
    "harvest_patches": ("event", _plain_case("harvest")),
    "negative_masks": ("event", _plain_case("negmasks")),
    "train_step, load_from_trainer, cnn_forward": ("host", _train_case()),
}


def sleep_cycles_per_ms():
    """torch.cuda._sleep counts device clock cycles: measured once with events"""
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    n = 20_000_000
    e0.record()
    torch.cuda._sleep(n)
    e1.record()
    torch.cuda.synchronize()
    return n / e0.elapsed_time(e1)


def run_stream_case(name, delay_ms, cycles_per_ms, control=False, quiet=None):
    """One case on a caller stream of its own.  quiet = "true" / "decoy": no delay, the inputs hold that scene throughout (the
    reference answers).  control: the library call runs on a second stream that nothing orders behind the producer.
    Returns dict(bytes, busy, call_ms)."""
    torch = _torch()
    proof, build = STREAM_CASES[name]
    bt = build()
    with _Env(bt.env):
        return _run_built(bt, proof, delay_ms, cycles_per_ms, control, quiet)


def _run_built(bt, proof, delay_ms, cycles_per_ms, control, quiet):
    torch = _torch()
    dev = lambda arrs: [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]   # noqa: E731
    true, decoy = dev(bt.true if quiet != "decoy" else bt.decoy), dev(bt.decoy if quiet != "true" else bt.true)
    stream, second = torch.cuda.Stream(), torch.cuda.Stream()
    for t, s in zip(bt.ins, decoy):
        t.copy_(s)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        bt.warm()   # the workspace of this shape exists from here on
    gc.collect()    # (a handle collected inside the timed part would synchronise the device in lg_destroy)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    t_enq = time.perf_counter()
    with torch.cuda.stream(stream):
        if quiet is None:
            torch.cuda._sleep(int(delay_ms * cycles_per_ms))
        ev.record(stream)
        for t, s in zip(bt.ins, true):
            t.copy_(s, non_blocking=True)
        with torch.cuda.stream(second if control else stream):
            t0 = time.perf_counter()
            enq_ms = (t0 - t_enq) * 1e3
            host, outs = bt.call()
            call_ms = (time.perf_counter() - t0) * 1e3
            pending = not ev.query()
            clones = [o.clone() for o in outs]
        for t, s in zip(bt.ins, decoy):
            t.copy_(s, non_blocking=True)
    torch.cuda.synchronize()
    busy = pending if proof == "event" else call_ms >= 0.5 * delay_ms
    parts = [_b(x) for x in list(host) + clones]
    return dict(bytes=b"|".join(parts), parts=parts, busy=bool(busy), call_ms=call_ms, enq_ms=enq_ms)


def stream_reference(name):
    """(answer on the true scene, answer on the decoy, quiescent call time in ms, the two answers in parts) of a case, on idle
    streams"""
    t = run_stream_case(name, 0.0, 1.0, quiet="true")
    d = run_stream_case(name, 0.0, 1.0, quiet="decoy")
    return t["bytes"], d["bytes"], max(t["call_ms"], d["call_ms"]), t["parts"], d["parts"]


def calibrate_delay(refs):
    """20 x the slowest quiescent call, at least 10 ms, at most 200 ms"""
    return min(200.0, max(10.0, 20.0 * max(r[2] for r in refs.values())))


def check_stream_case(name, ref, delay_ms, cycles_per_ms):
    """run the case; a case that cannot show a busy stream doubles the delay once.  -> dict for the JSON line / the assertion"""
    for d in (delay_ms, 2 * delay_ms):
        got = run_stream_case(name, d, cycles_per_ms)
        if got["busy"]:
            break
    wrong = [i for i, (p, t) in enumerate(zip(got["parts"], ref[3])) if p != t]
    return dict(case=name, busy=got["busy"], delay_ms=round(d, 2), call_ms=round(got["call_ms"], 3), enq_ms=round(got["enq_ms"], 3),
                ok=got["bytes"] == ref[0], wrong_parts=wrong, decoy_parts=[i for i in wrong if got["parts"][i] == ref[4][i]],
                decoy_differs=ref[0] != ref[1], saw_decoy=got["bytes"] == ref[1])


def classify_control(parts, ref):
    """the control's answer: "true", "decoy", "mixed" (a case of several library calls: each call's part is the true scene's or
    the decoy's -- a call that synchronises the device lets the later ones see the true scene) or "neither" """
    t, d = ref[3], ref[4]
    if len(parts) != len(t) or any(p != a and p != b for p, a, b in zip(parts, t, d)):
        return "neither"
    if all(p == b for p, b in zip(parts, d)):
        return "decoy"
    return "true" if all(p == a for p, a in zip(parts, t)) else "mixed"


def main_streams():
    """the child process of tests/test_gpu_stream_order.py: every case, then the control of the synchronising ones"""
    t0 = time.perf_counter()
    cpm = sleep_cycles_per_ms()
    refs = {n: stream_reference(n) for n in STREAM_CASES}
    delay = calibrate_delay(refs)
    print(json.dumps(dict(calibration=True, delay_ms=delay, cycles_per_ms=cpm, queues=os.environ.get("GPU_MAX_HW_QUEUES"),
                          quiescent_ms={n: round(r[2], 3) for n, r in refs.items()})), flush=True)
    for n in STREAM_CASES:
        print(json.dumps(check_stream_case(n, refs[n], delay, cpm)), flush=True)
    seen = {}
    for n, (proof, _) in STREAM_CASES.items():
        if proof != "host":
            continue
        got = run_stream_case(n, delay, cpm, control=True)
        # held: the second stream waited for the producer all the same (streams that share a hardware queue): the call then ran
        # beside the producer's copies and may have read the mask of one scene with the depth of the other
        seen[n] = dict(answer=classify_control(got["parts"], refs[n]), call_ms=round(got["call_ms"], 3),
                       held=got["call_ms"] >= 0.5 * delay)
    print(json.dumps(dict(control=True, saw_decoy=sum(v["answer"] == "decoy" for v in seen.values()),
                          held=sum(v["held"] for v in seen.values()), cases=len(seen), answers=seen,
                          seconds=round(time.perf_counter() - t0, 2))), flush=True)
    return 0


if __name__ == "__main__":
    if "--streams" in sys.argv:
        sys.exit(main_streams())
    sys.exit("usage: python -m tests.handle_cases --streams")
