"""Test-only restatement of the work plan of the persistent F(4x4,3x3) CNN kernels, to pick patch counts that reach every
plan (tests/test_gpu_cnn_regimes.py).

launch_wino4_rt (csrc/lg_cnn.hip, launch_wino4_rt) cuts a layer of N patches into items of 64 output channels x 32 tiles,
ceil(ntb / 8) * (cout / 64) of them per XCD, and launches gx workgroups per XCD (CUs / 8).  The kernel (lg_wino4_kernel,
"The tail") walks R full rounds of gx items and then rem left-over items, each split along the input channels over P
workgroups when the launcher finds the split worth its exchange.  With fewer items than workgroups the launcher shrinks
the grid: to items * P workgroups when it splits (R = 0), else to one workgroup per item (R = 1, rem = 0).  lg_cnn_run
cuts more than 8192 patches into slices of 8192 and runs each slice on its own.

Second half (device_plan and below): the plan of lg_select_grasp's pruned pass, whose grid comes from the host's bound
B * top_k and whose items come from the survivor count on the device, and the batches that
tests/test_gpu_cnn_prune_regimes.py runs to reach every class of it (tests/test_cnn_device_plan.py checks that they do)."""
from collections import OrderedDict

MAX_SLICE = 8192   # lg_cnn_run's max_slice


def model_layers(filters=(64, 128, 256)):
    """(cin, cout, width) of every F(4x4) layer of lg_cnn_plan's layer plan: channels padded to the 64-channel granule,
    layer 0 on 12 haloed input planes (the 9 features + 3 zero planes)."""
    out, cin, wi = [], 12, 32
    for f in filters:
        fp = (f + 63) // 64 * 64
        out.append((cin, fp, wi))
        out.append((fp, fp, wi))
        cin, wi = fp, wi // 2
    return out


def layer_plan(cin, cout, wi, n, num_cu):
    """(R, rem, P) of one layer of n <= MAX_SLICE patches as lg_wino4_kernel runs it; P = 1: left-over items run whole."""
    tp = (wi // 4) ** 2
    ntb = n * (tp // 32) if tp >= 32 else -(-n // (32 // tp))
    items8 = -(-ntb // 8) * (cout // 64)
    gx, p = num_cu // 8, 1
    rem = items8 if items8 < gx else items8 % gx
    if rem > 0:
        cap = min(gx // rem, 8, cin // 16)
        while 2 * p <= cap:
            p *= 2
    split = p > 1 and (cin // 4) * (p - 1) // p >= 26
    if items8 < gx:
        gx = items8 * (p if split else 1)
    r = items8 // gx
    return r, items8 - r * gx, p if split else 1


def slices(n):
    return [min(MAX_SLICE, n - o) for o in range(0, n, MAX_SLICE)]


def plan(layers, n, num_cu):
    """Per slice, per layer: (R, rem, P)."""
    return [[layer_plan(ci, co, wi, s, num_cu) for ci, co, wi in layers] for s in slices(n)]


def plan_class(r, rem, p):
    """The code paths a layer's plan takes: full rounds or none, a left-over item or none, and the split of the left-over item."""
    return (r >= 1, rem > 0, p)


def class_name(c):
    return f"{'R>=1' if c[0] else 'R=0'} {'tail' if c[1] else 'rem=0'} P{c[2]}"


EXTRA_N = (1, 2, 20, 640, 5120, 5121, 8192, 8193)


def pick_counts(layers, num_cu, n_max=MAX_SLICE + 1, extra=EXTRA_N):
    """-> (counts, first): the smallest n <= n_max of every (layer, reachable class) plus `extra`, sorted; and
    first[(layer, class)] = that smallest n."""
    first = OrderedDict()
    for n in range(1, min(n_max, MAX_SLICE) + 1):
        for li, (ci, co, wi) in enumerate(layers):
            first.setdefault((li, plan_class(*layer_plan(ci, co, wi, n, num_cu))), n)
    return sorted(set(first.values()) | {n for n in extra if n <= n_max}), first


def hit_classes(layers, counts, num_cu):
    """(layer, class) pairs that the given counts run, slices included."""
    hit = set()
    for n in counts:
        for sl in plan(layers, n, num_cu):
            for li, rp in enumerate(sl):
                hit.add((li, plan_class(*rp)))
    return hit


# --------------------------------------------------------------------------------------------- the device-count plan
# lg_select_grasp's pruned CNN pass (tests/test_gpu_cnn_prune_regimes.py): the launcher sizes the grid for the host's upper
# bound n_host = B * top_k with no split, and the kernel recomputes its item plan from the count n_dev the device produced
# (lg_wino4_kernel, "Patch count").  The plan is a function of both numbers.
def _ntb(wi, n):
    tp = (wi // 4) ** 2
    return n * (tp // 32) if tp >= 32 else -(-n // (32 // tp))


def device_plan(cin, cout, wi, n_host, n_dev, num_cu):
    """(R, rem, idle workgroups) of one layer of a slice with n_host <= MAX_SLICE patch slots of which n_dev <= n_host hold a
    patch.  The grid is the unsplit host plan's (fewer items than workgroups shrink it to one workgroup per item); ntb, the
    item list, R and rem follow from n_dev; no item is split (P = 1); a workgroup without an item leaves at once (idle).
    num_cu is what the launcher takes: all CUs of the device."""
    assert 0 <= n_dev <= n_host <= MAX_SLICE
    items8 = -(-_ntb(wi, n_host) // 8) * (cout // 64)
    gx = min(num_cu // 8, items8)
    llen = -(-_ntb(wi, n_dev) // 8) * (cout // 64)
    r = llen // gx
    rem = llen - r * gx
    return r, rem, 8 * (gx - rem) if r == 0 else 0


def device_class(r, rem, idle):
    """Full rounds or none, a left-over round or none, idle workgroups or none, and no item at all (llen = 0)."""
    return (r >= 1, rem > 0, idle > 0, r == 0 and rem == 0)


def device_class_name(c):
    if c[3]:
        return "llen=0 (all idle)"
    return f"{'R>=1' if c[0] else 'R=0'} {'tail' if c[1] else 'rem=0'} {'idle' if c[2] else 'no idle'}"


def device_slices(n_host, n_dev):
    """lg_cnn_run's slices of a pruned pass: (patch slots, patches) of each -- every slice of the host's bound is launched and
    takes what of the device's count lies in it."""
    return [(min(MAX_SLICE, n_host - o), max(0, min(n_dev - o, MAX_SLICE, n_host - o))) for o in range(0, n_host, MAX_SLICE)]


def device_classes(layers, n_host, n_dev, num_cu):
    """(layer, class) pairs that a pruned pass of n_host slots and n_dev patches runs, slices included."""
    return {(li, device_class(*device_plan(ci, co, wi, nh, nd, num_cu)))
            for nh, nd in device_slices(n_host, n_dev) for li, (ci, co, wi) in enumerate(layers)}


# How the GPU test steers n_dev: a batch of B frames at top_k = K holds `e` frames with an empty uint8 mask (all K candidates
# tie at the constant tile's score: K survivors) and B - e leaf frames on which only candidate 0 survives (1 survivor).  A
# frame with one candidate is not rescored: K = 1 gives no survivor at all.
def survivors_of(b, k, e):
    assert 0 <= e <= b and 1 <= k <= 64
    return 0 if k == 1 else e * k + (b - e)


def compose(n_host, n_dev):
    """(B, K, e) with B * K = n_host and survivors_of(B, K, e) = n_dev, of the fewest frames; None where there is none."""
    for k in range(64, 0, -1):
        if n_host % k:
            continue
        b = n_host // k
        if k == 1:
            if n_dev == 0:
                return b, 1, 0
        elif n_dev >= b and (n_dev - b) % (k - 1) == 0 and (n_dev - b) // (k - 1) <= b:
            return b, k, (n_dev - b) // (k - 1)
    return None


def pick_device_pairs(layers, num_cu, n_host_max=1300):
    """-> first[(layer, class)] = the smallest (n_host, n_dev), n_host <= n_host_max, that `compose` can make and that runs
    the layer in that class.  Every layer reaches four classes: no item; items on some workgroups only (R = 0: the others
    idle); full rounds alone; full rounds and a left-over round."""
    first = OrderedDict()
    want = 4 * len(layers)
    for n_host in range(1, n_host_max + 1):
        devs = sorted({survivors_of(n_host // k, k, e) for k in range(1, 65) if n_host % k == 0 for e in range(n_host // k + 1)})
        for n_dev in devs:
            for li, (ci, co, wi) in enumerate(layers):
                first.setdefault((li, device_class(*device_plan(ci, co, wi, n_host, n_dev, num_cu))), (n_host, n_dev))
        if len(first) == want:
            break
    return first


# (name, B, K, e) beside the picker's pairs: no survivor, one, all of them, odd counts that fill no tile block of the 16 x 16
# (2 patches) and 8 x 8 layers (8 patches), half of a larger bound (full rounds and a left-over round on a grid that the
# count does not fill evenly), and the slice boundary -- 8192 of 8420 slots (the second slice runs on nothing),
# 8193 (one patch in it) and 8301 (109 = 13 * 8 + 5).
EXTRA_BATCHES = (("none", 3, 1, 1), ("one", 1, 20, 0), ("all", 3, 20, 3), ("all, odd", 3, 7, 3), ("17", 5, 7, 2),
                 ("57", 9, 13, 4), ("420", 40, 20, 20), ("8192", 421, 20, 409), ("8193", 129, 64, 128), ("8301", 416, 20, 415))


def prune_batches(layers, num_cu):
    """[(name, B, K, e)] of the GPU test: EXTRA_BATCHES and a composition of every pair the picker returns."""
    out = list(EXTRA_BATCHES)
    for nh, nd in sorted(set(pick_device_pairs(layers, num_cu).values())):
        b, k, e = compose(nh, nd)
        if (b, k, e) not in [t[1:] for t in out]:
            out.append((f"{nh}/{nd}", b, k, e))
    return out


def device_table(layers, batches, num_cu):
    lines = [f"CUs {num_cu}; (R,rem,idle) per layer (cin->cout@width): " +
             ", ".join(f"L{i} {ci}->{co}@{wi}" for i, (ci, co, wi) in enumerate(layers))]
    for name, b, k, e in batches:
        nh, nd = b * k, survivors_of(b, k, e)
        per = " | ".join(" ".join("({},{},{})".format(*device_plan(ci, co, wi, h, d, num_cu)) for ci, co, wi in layers)
                         for h, d in device_slices(nh, nd))
        lines.append(f"B {b:4d} top_k {k:2d} empty {e:3d}: n_host {nh:5d} n_dev {nd:5d}: {per}")
    return "\n".join(lines)


def table(layers, counts, num_cu):
    lines = [f"CUs {num_cu}; per layer (cin->cout@width): " + ", ".join(f"L{i} {ci}->{co}@{wi}" for i, (ci, co, wi) in
                                                                            enumerate(layers))]
    for n in counts:
        per = " | ".join(" ".join(f"({r},{rem},{p})" for r, rem, p in sl) for sl in plan(layers, n, num_cu))
        lines.append(f"N {n:5d}: {per}")
    return "\n".join(lines)
