"""Step E of the orientation kernel in two levels (lg_orient.hip): a row is tested against the rows of its own block of 16
first, and the survivors of a chain against each other afterwards.  Re-stated here with the kernel's integer comparisons and
compared with the all-rows test in exact rational arithmetic: the vertex flags of both chains must be the same, row by row.
The all-rows test is stated twice, with slopes as Fractions and as the chord definition in integers; the two are held against
each other, and the integer form serves where the Fractions would take seconds (more than 64 rows)."""
from fractions import Fraction

import numpy as np
import pytest

OBLK = 16


def vertex(X, rows, j, left):
    """the kernel's hull_vertex: rows[j] against rows[0 .. len), integer cross-multiplied slope comparisons"""
    if j == 0 or j == len(rows) - 1:
        return True
    i = rows[j]
    xi = int(X[i])
    p, q = xi - int(X[rows[0]]), i - rows[0]
    for a in range(1, j):
        r = rows[a]
        qq, pp = i - r, xi - int(X[r])
        if (pp * q > p * qq) if left else (pp * q < p * qq):
            p, q = pp, qq
    rb = rows[j + 1]
    p2, q2 = int(X[rb]) - xi, rb - i
    for c in range(j + 2, len(rows)):
        r = rows[c]
        qq, pp = r - i, int(X[r]) - xi
        if (pp * q2 < p2 * qq) if left else (pp * q2 > p2 * qq):
            p2, q2 = pp, qq
    return (p * q2 < p2 * q) if left else (p * q2 > p2 * q)


def two_level(L, R, blk=OBLK):
    n = len(L)
    out = []
    for X, left in ((L, True), (R, False)):
        surv = []
        for b0 in range(0, n, blk):
            rows = list(range(b0, min(b0 + blk, n)))
            surv += [rows[j] for j in range(len(rows)) if vertex(X, rows, j, left)]
        flags = np.zeros(n, bool)
        for k in range(len(surv)):
            flags[surv[k]] = vertex(X, surv, k, left)
        out.append(flags)
    for i in (0, n - 1):   # the chains meet at the top and bottom rows: a shared end point stays with the left chain
        if L[i] == R[i]:
            out[1][i] = False
    return out[0], out[1], None


def all_rows_chords(L, R):
    """the definition itself, in integers: row i is a strict vertex of the left chain iff it lies strictly left of every chord
    from a row above to a row below, x_i (c - a) < x_a (c - i) + x_c (i - a); right chain mirrored"""
    n = len(L)
    out = []
    for X, sgn in ((np.asarray(L, np.int64), 1), (np.asarray(R, np.int64), -1)):
        flags = np.ones(n, bool)
        for i in range(1, n - 1):
            qa, qc = i - np.arange(i), np.arange(1, n - i)
            lhs = sgn * X[i] * (qa[:, None] + qc[None, :])
            rhs = sgn * (X[:i, None] * qc[None, :] + X[None, i + 1:] * qa[:, None])
            flags[i] = bool((lhs < rhs).all())
        out.append(flags)
    for i in (0, n - 1):
        if L[i] == R[i]:
            out[1][i] = False
    return out[0], out[1]


def all_rows_exact(L, R):
    """every row against every other row, slopes as Fractions: strict vertex iff max arriving < min leaving (left chain).
    Past 64 rows the chords stand in (the same vertices, see test_the_two_all_rows_tests_agree): Fractions take seconds there"""
    if len(L) > 64:
        return all_rows_chords(L, R)
    return all_rows_fractions(L, R)


def all_rows_fractions(L, R):
    n = len(L)
    out = []
    for X, sgn in ((L, 1), (R, -1)):
        flags = np.ones(n, bool)
        for i in range(1, n - 1):
            arrive = max(Fraction(sgn * (int(X[i]) - int(X[a])), i - a) for a in range(i))
            leave = min(Fraction(sgn * (int(X[c]) - int(X[i])), c - i) for c in range(i + 1, n))
            flags[i] = arrive < leave
        out.append(flags)
    for i in (0, n - 1):
        if L[i] == R[i]:
            out[1][i] = False
    return out[0], out[1]


def _profiles(n, rng):
    i = np.arange(n)
    out = {}
    for k in range(3):
        L = rng.integers(0, 400, n)
        out[f"random {k}"] = (L, L + rng.integers(0, 300, n))
    L = rng.integers(0, 3, n)
    out["random, three values"] = (L, L + rng.integers(0, 3, n))
    c = (n - 1) / 2.0
    arc = np.sqrt(np.clip((n / 2.0 + 1) ** 2 - (i - c) ** 2, 0, None))
    out["convex arc with jitter"] = (np.round(500 - arc + rng.integers(0, 2, n)).astype(int),
                                     np.round(500 + arc - rng.integers(0, 2, n)).astype(int))
    out["convex arc"] = (np.round(500 - arc).astype(int), np.round(500 + arc).astype(int))
    L, R = np.full(n, 100), np.full(n, 300)
    dents = rng.random(n) < 0.15
    out["constant with dents"] = (L + dents * rng.integers(1, 9, n), R - dents * rng.integers(1, 9, n))
    out["constant"] = (np.full(n, 7), np.full(n, 7))            # one column: every row is collinear, the chains coincide
    out["diamond"] = (500 - np.minimum(i, n - 1 - i), 500 + np.minimum(i, n - 1 - i))
    out["staircase"] = (100 + (i // 5) * 4, 400 + (i // 7) * 6)
    out["slanted line"] = (10 + 3 * i, 10 + 3 * i)
    out["bumps outwards"] = (np.full(n, 100) - dents * rng.integers(1, 9, n), np.full(n, 300) + dents * rng.integers(1, 9, n))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 32, 33, 300])
def test_two_levels_give_the_all_rows_vertices(n):
    rng = np.random.default_rng(50 + n)
    seen = 0
    for name, (L, R) in _profiles(n, rng).items():
        gl, gr, _ = two_level(L, R)
        el, er = all_rows_exact(L, R)
        assert (gl == el).all() and (gr == er).all(), (name, n, np.flatnonzero(gl != el), np.flatnonzero(gr != er))
        seen += int(el.sum()) + int(er.sum())
    assert seen >= 2 * len(_profiles(n, rng)) or n == 1


def test_the_two_all_rows_tests_agree():
    for n, names in ((17, None), (33, None), (64, None), (300, ("random 0", "convex arc with jitter", "constant with dents"))):
        for name, (L, R) in _profiles(n, np.random.default_rng(7 * n)).items():
            if names is None or name in names:
                fl, fr = all_rows_fractions(L, R)
                cl, cr = all_rows_chords(L, R)
                assert (fl == cl).all() and (fr == cr).all(), (name, n)


@pytest.mark.parametrize("blk", [8, 16, 64])
def test_any_block_size(blk):
    rng = np.random.default_rng(blk)
    for n in (blk - 1, blk, blk + 1, 3 * blk + 2):
        for name, (L, R) in _profiles(n, rng).items():
            gl, gr, _ = two_level(L, R, blk)
            el, er = all_rows_exact(L, R)
            assert (gl == el).all() and (gr == er).all(), (name, n, blk)


def test_first_level_prunes():
    """on an arc most rows fall at the first level already (what the two levels are for), and none that is a vertex"""
    n = 300
    L, R = _profiles(n, np.random.default_rng(1))["convex arc"]
    surv = [b0 + j for b0 in range(0, n, OBLK) for j in range(min(OBLK, n - b0))
            if vertex(L, list(range(b0, min(b0 + OBLK, n))), j, True)]
    assert len(surv) < n // 2
    el, _ = all_rows_exact(L, R)
    assert set(np.flatnonzero(el)) <= set(surv)
