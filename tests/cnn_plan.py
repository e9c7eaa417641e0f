"""Test-only restatement of the work plan of the persistent F(4x4,3x3) CNN kernels, to pick patch counts that reach every
plan (tests/test_gpu_cnn_regimes.py).

launch_wino4_rt (csrc/lg_cnn.hip, launch_wino4_rt) cuts a layer of N patches into items of 64 output channels x 32 tiles,
ceil(ntb / 8) * (cout / 64) of them per XCD, and launches gx workgroups per XCD (CUs / 8).  The kernel (lg_wino4_kernel,
"The tail") walks R full rounds of gx items and then rem left-over items, each split along the input channels over P
workgroups when the launcher finds the split worth its exchange.  With fewer items than workgroups the launcher shrinks
the grid: to items * P workgroups when it splits (R = 0), else to one workgroup per item (R = 1, rem = 0).  lg_cnn_run
cuts more than 8192 patches into slices of 8192 and runs each slice on its own."""
from collections import OrderedDict

MAX_SLICE = 8192   # lg_cnn_run's max_slice


def model_layers(filters=(64, 128, 256)):
    """(cin, cout, width) of every F(4x4) layer of lg_cnn_upload's layer plan: channels padded to the 64-channel granule,
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


def table(layers, counts, num_cu):
    lines = [f"CUs {num_cu}; per layer (cin->cout@width): " + ", ".join(f"L{i} {ci}->{co}@{wi}" for i, (ci, co, wi) in
                                                                            enumerate(layers))]
    for n in counts:
        per = " | ".join(" ".join(f"({r},{rem},{p})" for r, rem, p in sl) for sl in plan(layers, n, num_cu))
        lines.append(f"N {n:5d}: {per}")
    return "\n".join(lines)
