"""Tie-ladder tableaux: inputs on which the order of the eps-argmin tree decides the winner.

compare(x, y, eps = 1e-9) is not transitive (v, v + 0.6 eps, v + 1.2 eps tie pairwise, not end to
end), so on values that form eps-chains the winner of an argmin depends on the combine order:
32-lane shuffles, 512-thread tiles, then the pass over the tile winners (oracle/simplex_oracle.c,
the restatement of reduction.cu:10-104).  The generators below put every value on a grid of
q = 0.125e-9 (0.25e-9 for `disjoint`) around 1.0, so the column sums that form the objective row
and the ratios b_i / a_ie land in such chains, pivot after pivot.

`census` counts, with the oracle alone, how many pivots of an instance are decided by the tree
order; tests/test_tie_ladders.py holds the floors, tests/test_gpu_tie_ladders.py runs the same
instances through every selection path of the engine.

Census of the committed cases (k pivots each; "sens" = the oracle's choice differs from np.argmin
or from a left-to-right eps-scan, "win" = the winner has a second, different value inside its
eps-window; entering / ratio):

    case      generator(n, m, g) seed        k  done  sens     argmin   scan     win
    D-1       disjoint(40, 1100, 24) 1      40    40  38 / 35  35 / 27  30 / 26  39 / 40
    D-2       disjoint(40, 1100, 24) 2      40    40  36 / 33  35 / 29  30 / 23  38 / 40
    O-1       overlap(200, 1100, 12) 1     150   150  26 / 32  23 / 29  21 / 14  39 / 43
    O-2       overlap(200, 1100, 12) 2     150   150  40 / 22  38 / 21  30 / 10  43 / 35
    O-small   overlap(40, 333, 16) 1        40    40  10 / 12   8 / 11   9 /  8  13 / 14
    W64       wide(32672, 48, 3) 1          30    30  28 /  9  26 /  8  20 /  3  30 / 13
    W65       wide(32673, 48, 3) 1          30    30  27 / 11  27 /  8  20 /  7  30 / 15
    W160      wide(81824, 48, 3) 1          30    30  28 / 15  27 / 10  18 /  9  30 / 19
    W161      wide(81825, 48, 3) 1          30    30  29 / 13  28 / 10  20 /  6  30 / 16
    W65x2-1   wide(31649, 560, 3) 1         40    40  40 / 21  40 / 20  34 / 10  40 / 29
    W65x2-2   wide(31649, 560, 3) 2         40    40  40 / 22  39 / 14  35 / 15  40 / 32
    O-tiles-1 overlap(1400, 1100, 12) 1    100   100  28 / 19  27 / 16  21 /  9  30 / 25
    O-tiles-2 overlap(1400, 1100, 12) 2    100   100  35 / 22  34 / 21  27 / 10  36 / 27

tile_merge_census (pivots at which merging the TILE winners left to right / right to left picks
another index than the reference's pass 2; entering | ratio):
    D-1 0/0 | 0/39    D-2 0/0 | 0/36    O-1 0/0 | 0/26    O-2 0/0 | 1/23    O-small 0/0 | 0/0
    O-tiles-1 1/26 | 1/13    O-tiles-2 2/34 | 0/15
    W64 7/29 | 0/0    W65 3/30 | 0/0    W160 5/30 | 0/0    W161 9/29 | 0/0
    W65x2-1 0/40 | 0/3    W65x2-2 4/40 | 0/6

(a generated instance, generate(200, 1100, 21100, 1, 100), 60 pivots: win 0 / 0, ratio sens 0; its
40 entering-sensitive pivots are exact ties between slack columns at -1.0, where the tree picks
among equal values.)  Whole solves of D-1 and O-small with the
ladder cost vector `cost_vector`: see WHOLE_SOLVES below.

Whole LPs for the batched-solve kernels (BATCH_CASES: sized for the LDS and the workspace class of
sx_batch.hip, cost vector cost_vector(n, seed); tests/test_gpu_batch_ladders.py runs them through
both batch entries).  census_two_phase, per phase (k = the oracle's pivots of the phase, all of
them replayed), the columns of the two tables above:

    case     generator(n, m, g) seed          phase    k  sens       argmin     scan       win        lin/rev enter | ratio
    B-small  overlap(40, 60, 8, spare=8) 1        1  133   23 /  13   20 /  12   22 /   5   11 /  16  0/0   | 0/0
                                                  2   57    9 /   5    6 /   5    7 /   3   11 /   5  0/0   | 0/0
    B-wide3  wide(1100, 12, 3, spare=4) 2         1   13   10 /   1   10 /   1    6 /   1    9 /   2  0/9   | 0/0
                                                  2   15   10 /   1    9 /   1    4 /   0   10 /   3  0/7   | 0/0
    B-w1024  wide(1000, 12, 3, spare=4) 2         1   12    8 /   1    8 /   1    5 /   1    8 /   2  0/8   | 0/0
                                                  2   14    8 /   1    8 /   0    5 /   1   10 /   3  0/6   | 0/0
    B-w1025  wide(1001, 12, 3, spare=4) 1         1   12   10 /   2    9 /   1    9 /   2    8 /   2  0/8   | 0/0
                                                  2   15   10 /   1    8 /   1    6 /   0   12 /   3  0/7   | 0/0
    B-ws     overlap(40, 600, 12) 1               1  880  550 / 156  543 / 137  520 /  87  168 / 211  0/455 | 0/100
                                                  2   41   26 /  11   24 /  11   19 /   6   31 /  14  0/26  | 0/11
    B-trim   disjoint(20, 560, 24) 1              1  560  518 /  17  518 /  16  516 /  10   18 /  20  0/472 | 0/14
                                                  2   20   16 /   0   13 /   0   13 /   0   19 /   0  0/0   | 0/0
    O-small  overlap(40, 333, 16) 1               1  670  250 /  43  244 /  34  246 /  27   31 /  51  0/0   | 0/0
                                                  2   73   10 /  18    8 /  14    8 /  10   15 /  26  0/0   | 0/0
    B-w65t   wide(32745, 12, 3, spare=4) 1        1   13   11 /   1   10 /   1    9 /   1    9 /   1  0/9   | 0/0
                                                  2   14    8 /   2    6 /   1    4 /   1    9 /   3  0/6   | 0/0

Whole solves with another selection rule (standin_two_phase): np.argmin ends at another basis on
every case but B-trim; the tile winners merged right to left end at another basis on B-wide3,
B-w1024, B-w1025, B-w65t and B-ws and change nothing on B-small and O-small (no pivot of theirs is decided
between tiles).  On B-trim both rules end at the oracle's basis after the oracle's pivot counts, with
other bits in the objective and the objective row -- and at another basis mid-solve (after 1 and 3
pivots), which is what the capped prefixes of the GPU tests see.
"""
import numpy as np

import oracle

EPS = 1e-9
DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------ generators: (A m x n, b)
def disjoint(n, m, g, seed, q=0.25e-9):
    """column j: ones in its own g rows; a "trim" below eps (never eligible as a pivot) in one of
    the spare rows turns the column sums into a ladder"""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    rows = rng.permutation(m)
    for j in range(n):
        A[rows[j * g:(j + 1) * g], j] = 1.0
    b = 1.0 + q * rng.integers(0, 8, size=m)
    free = rows[n * g:]
    tr = free[:max(1, len(free) // 2)]
    for j in range(n):
        A[rng.choice(tr), j] += q * rng.integers(0, 4)
    return A, b


def overlap(n, m, g, seed, q=0.125e-9, levels=16, spare=32):
    """the columns' supports overlap, so the pending pivots of a batch act on later decisions"""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    b = 1.0 + q * rng.integers(0, levels, size=m)
    body = m - spare
    for j in range(n):
        A[rng.choice(body, size=g, replace=False), j] = 1.0
        A[body + rng.integers(0, spare), j] += q * rng.integers(0, 8)
    return A, b


def wide(n, m, g, seed, q=0.125e-9, levels=16, spare=8):
    """few rows, tens of thousands of columns: many objective tiles"""
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    b = 1.0 + q * rng.integers(0, levels, size=m)
    body = m - spare
    rows = np.argsort(rng.random((n, body)), axis=1)[:, :g]
    for t in range(g):
        A[rows[:, t], np.arange(n)] = 1.0
    A[body + rng.integers(0, spare, size=n), np.arange(n)] += q * rng.integers(0, 8, size=n)
    return A, b


GENERATORS = {"disjoint": disjoint, "overlap": overlap, "wide": wide}

# name -> (generator, (n, m, g), seed, pivots k, entering-sensitive floor, ratio-sensitive floor).
# The floors are conditions on the inputs (a seed that misses one is replaced, the floor stays).
CASES = {
    "D-1": ("disjoint", (40, 1100, 24), 1, 40, 30, 30),
    "D-2": ("disjoint", (40, 1100, 24), 2, 40, 30, 30),
    "O-1": ("overlap", (200, 1100, 12), 1, 150, 20, 16),
    "O-2": ("overlap", (200, 1100, 12), 2, 150, 20, 16),
    "O-small": ("overlap", (40, 333, 16), 1, 40, 8, 8),       # a partial 16-row strip, one ratio tile
    # structural columns over three objective tiles (D and O keep theirs inside tile 0)
    "O-tiles-1": ("overlap", (1400, 1100, 12), 1, 100, 20, 16),
    "O-tiles-2": ("overlap", (1400, 1100, 12), 2, 100, 20, 16),
    # n + 2m = 64, 65, 160 and 161 objective tiles of 512 columns
    "W64": ("wide", (32768 - 96, 48, 3), 1, 30, 25, 5),
    "W65": ("wide", (32769 - 96, 48, 3), 1, 30, 25, 5),
    "W160": ("wide", (81920 - 96, 48, 3), 1, 30, 25, 5),
    "W161": ("wide", (81921 - 96, 48, 3), 1, 30, 25, 5),
    # 65 objective tiles, rows on two 512-aligned shards
    "W65x2-1": ("wide", (31649, 560, 3), 1, 40, 35, 15),
    "W65x2-2": ("wide", (31649, 560, 3), 2, 40, 35, 15),
}


# Where the order in which TILE winners are merged decides (tile_merge_census): the side on which
# at least the case's floor of pivots changes when the tile winners are merged right to left.  D and
# O: the ratio side (rows over 3 tiles; their ladder columns all lie in objective tile 0); O-tiles
# and the wide cases: the entering side.  O-small has one ratio tile and one ladder tile: lanes only.
TILE_MERGE = {"D-1": "ratio", "D-2": "ratio", "O-1": "ratio", "O-2": "ratio", "O-tiles-1": "enter", "O-tiles-2": "enter",
              "W64": "enter", "W65": "enter", "W160": "enter", "W161": "enter", "W65x2-1": "enter", "W65x2-2": "enter"}

# whole two-phase solves with the cost vector cost_vector(n, 1): the oracle's (status, (phase-1
# pivots, phase-2 pivots)); every artificial variable has to leave, so phase 1 takes >= m pivots
WHOLE_SOLVES = {"D-1": (oracle.FEASIBLE, (1100, 40)), "O-small": (oracle.FEASIBLE, (670, 73))}


def make(name):
    """(A, b, k) of a committed case"""
    gen, args, seed, k, _, _ = CASES[name]
    A, b = GENERATORS[gen](*args, seed)
    return A, b, k


# Whole LPs for the resident workgroups of the batched solve (sx_batch.hip wg_argmin): name ->
# (generator, (n, m, g), generator keywords, seed, batch class (2 LDS, 1 workspace), the oracle's
# (phase-1, phase-2) pivots).  The cost vector is cost_vector(n, seed); every solve ends FEASIBLE.
BATCH_CASES = {
    "B-small": ("overlap", (40, 60, 8), {"spare": 8}, 1, 2, (133, 57)),   # one tile each side: the lane tree
    "B-wide3": ("wide", (1100, 12, 3), {"spare": 4}, 2, 2, (13, 15)),     # 3 entering tiles in both phases, in LDS
    "B-w1024": ("wide", (1000, 12, 3), {"spare": 4}, 2, 2, (12, 14)),     # n + 2m = 1024: exactly 2 full tiles
    "B-w1025": ("wide", (1001, 12, 3), {"spare": 4}, 1, 2, (12, 15)),     # n + 2m = 1025: the third tile holds one value
    "B-ws": ("overlap", (40, 600, 12), {}, 1, 1, (880, 41)),              # ratio over 2 row tiles, entering over 3
    "B-trim": ("disjoint", (20, 560, 24), {}, 1, 1, (560, 20)),           # sub-eps trims, ratio over 2 tiles
    "O-small": ("overlap", (40, 333, 16), {}, 1, 1, (670, 73)),           # (CASES["O-small"], WHOLE_SOLVES)
    # n + 2m = 32769: 65 entering tiles (64 in phase 2), so pass 2 combines winners across its 32-lane halves and waves
    "B-w65t": ("wide", (32769 - 24, 12, 3), {"spare": 4}, 1, 1, (13, 14)),
}

# Floors of census_two_phase per case: {(phase, key): floor}, conditions on the inputs like CASES'.
BATCH_FLOORS = {
    "B-small": {(1, "enter_sensitive"): 15, (1, "ratio_sensitive"): 10, (2, "enter_sensitive"): 5, (2, "ratio_sensitive"): 3},
    "B-wide3": {(1, "enter_rev"): 6, (2, "enter_rev"): 4},
    "B-w1024": {(1, "enter_rev"): 5, (2, "enter_rev"): 4},
    "B-w1025": {(1, "enter_rev"): 5, (2, "enter_rev"): 4},
    "B-ws": {(1, "ratio_rev"): 60, (2, "ratio_rev"): 6, (1, "enter_rev"): 300, (2, "enter_rev"): 15},
    "B-trim": {(1, "enter_sensitive"): 400, (1, "ratio_rev"): 10},
    "O-small": {},
    "B-w65t": {(1, "enter_rev"): 5, (2, "enter_rev"): 4},
}


def make_batch(name, seed=None):
    """(A, b, c) of a BATCH_CASES case; `seed` other than the committed one: a neighbour of the
    same shape (the floors are measured on the committed seed only)"""
    gen, args, kw, seed0, _, _ = BATCH_CASES[name]
    seed = seed0 if seed is None else seed
    A, b = GENERATORS[gen](*args, seed, **kw)
    return A, b, cost_vector(args[0], seed)


def phase1_state(A, b):
    """the canonical phase-1 tableau (T, d, base) of (A, b)"""
    T, d, base = oracle.build_phase1(A, b)
    oracle.update_objective(T, d, base)
    return T, d, base


def cost_vector(n, seed, q=0.125e-9):
    """c = -(1 + q k_j): a ladder for phase 2's objective row"""
    return -(1.0 + q * np.random.default_rng(seed).integers(0, 8, size=n))


def ladder_vector(L):
    """an argmin input that is one ladder: -(3 + 0.125e-9 k), k in 0..15, at every position"""
    return -(3.0 + 0.125e-9 * np.random.default_rng(L).integers(0, 16, size=L))


# ------------------------------------------------------------------ eligibility boundaries of compare()
BOUNDARY = {"below": np.nextafter(1e-9, 0), "at": 1e-9, "above": np.nextafter(1e-9, 1)}


def boundary_state(kind, x):
    """A hand-built 20 x (1 + 6 + 40) phase-1 state (T, d, base) for one pivot.
    kind "entry": the entering column's (column 3, reduced cost -2) largest entry is x, in row 11;
    every other entry of the column is <= 0.5e-9.  The oracle: UNBOUNDED for x < 1e-9, else a pivot
    on that entry.
    kind "cost": the most negative reduced cost is -x (column 4, ordinary positive entries), every
    other one is >= 0.  The oracle: the phase ends for x < 1e-9, else a pivot."""
    m, n = 20, 6
    N = 1 + n + 2 * m
    rng = np.random.default_rng(20)
    T = np.zeros((m, N))
    T[:, 0] = rng.integers(1, 9, size=m).astype(np.float64)
    T[:, 1:1 + n] = rng.integers(-4, 5, size=(m, n)).astype(np.float64)
    T[np.arange(m), 1 + n + np.arange(m)] = 1.0
    T[np.arange(m), 1 + n + m + np.arange(m)] = 1.0
    base = (n + m + np.arange(m)).astype(np.int32)
    d = np.zeros(N)
    d[1:1 + n] = [0.5, 1.0, 3.0, 2.0, 0.25, 0.0]
    d[1 + n:1 + n + m] = 0.125 * rng.integers(0, 8, size=m)
    if kind == "entry":
        d[1 + 3] = -2.0
        d[1 + 1] = -1.0
        col = -rng.integers(0, 4, size=m).astype(np.float64)
        col[2], col[7], col[15] = 0.5e-9, -0.0, BOUNDARY["below"] / 2
        col[11] = x
        T[:, 1 + 3] = col
    else:
        assert kind == "cost"
        T[:, 1 + 4] = rng.integers(1, 6, size=m).astype(np.float64)
        d[1 + 4] = -x
    return T, d, base


def boundary_lp(kind, x):
    """The same boundaries as a whole LP (A 20 x 6, b, c) for the batch entries, which take no
    tableau.  b: positive integers; A: multiples of 1/128 with every column sum below 1, so phase 1
    is exactly m slack pivots (each on a 1.0, every other entry of the column 0) that leave
    [b | A | I] as built, and phase 2's first decision falls on the raw data.
    kind "entry": the column of the largest cost (column 3) has x in row 11 and otherwise entries
    <= 0.5e-9.  The oracle: UNBOUNDED after (20, 0) pivots for x < 1e-9, else phase 2 pivots.
    kind "cost": the only positive cost is x (column 4).  The oracle: FEASIBLE after (20, 0) pivots
    for x < 1e-9, else (20, 1) with column 4 basic."""
    m, n = 20, 6
    rng = np.random.default_rng(20)
    b = rng.integers(1, 9, size=m).astype(np.float64)
    A = rng.integers(0, 6, size=(m, n)) / 128.0
    c = -(1.0 + rng.integers(0, 4, size=n).astype(np.float64))
    if kind == "entry":
        c[3], c[1] = 2.0, 1.0
        col = -rng.integers(0, 4, size=m) / 128.0
        col[2], col[7], col[15] = 0.5e-9, -0.0, BOUNDARY["below"] / 2
        col[11] = x
        A[:, 3] = col
    else:
        assert kind == "cost"
        A[:, 4] = rng.integers(1, 6, size=m) / 128.0
        c[4] = x
    return A, b, c


# ------------------------------------------------------------------ the plain rules
def ratios(T, e):
    """createIndicatorsVector: b_i / a_ie where a_ie >= 1e-9, else DBL_MAX"""
    col = T[:, 1 + e]
    ok = col >= EPS
    out = np.full(T.shape[0], DBL_MAX)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        out[ok] = T[ok, 0] / col[ok]
    return out


def _negative(x):
    """compare(x, 0) < 0"""
    return bool(x < 0 and not abs(x) < EPS)


def eps_scan(v):
    """left-to-right scan that keeps the incumbent unless compare(x, best) < 0"""
    best = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while True:
            rest = v[best + 1:]
            hit = np.flatnonzero((rest < v[best]) & ~(np.abs(rest - v[best]) < EPS))
            if hit.size == 0:
                return best
            best += 1 + int(hit[0])


def window(v, i, width=EPS):
    """indices (other than ties in value) within `width` of v[i]: its eps-window"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.flatnonzero((np.abs(v - v[i]) < width) & (v != v[i]))


_CENSUS_KEYS = ("enter_argmin", "enter_scan", "enter_sensitive", "enter_window",
                "ratio_argmin", "ratio_scan", "ratio_sensitive", "ratio_window")
_MERGE_KEYS = ("enter_lin", "enter_rev", "ratio_lin", "ratio_rev")


def _replay(T, d, base, k, count):
    """up to k pivots (k < 0: until the phase ends) of the state (T, d, base), in place, with
    oracle.pivot; before each pivot is applied, count(v, e, rv, r) sees the entering vector d[1:],
    the oracle's entering index, the ratio vector of that column and the oracle's leaving row.
    Returns (pivots taken, the status that ended the replay)."""
    done = 0
    while k < 0 or done < k:
        v = d[1:].copy()
        e_pred = oracle.argmin(v)[0]
        rv = ratios(T, e_pred) if e_pred >= 0 else None
        st, e, r = oracle.pivot(T, d, base)
        if st != oracle.NOT_ENDED:
            return done, st
        assert e == e_pred and r == oracle.argmin(rv)[0]
        done += 1
        count(v, e, rv, r)
    return done, oracle.PIVOT_CAP


def _count_census(out):
    def count(v, e, rv, r):
        for side, vec, win in (("enter", v, e), ("ratio", rv, r)):
            a, s = int(np.argmin(vec)) != win, eps_scan(vec) != win
            out[side + "_argmin"] += a
            out[side + "_scan"] += s
            out[side + "_sensitive"] += a or s
            out[side + "_window"] += window(vec, win).size > 0
    return count


def census(A, b, k):
    """Replay k pivots of (A, b)'s phase 1 with oracle.pivot and count the pivots the combine tree
    decides.  Per side (entering: d[1:]; ratio: the ratio vector of the entering column):
    `*_argmin` / `*_scan`: the oracle's choice differs from np.argmin / from eps_scan;
    `*_sensitive`: from either; `*_window`: the winner has a second, different value inside its
    eps-window.  `done`: pivots taken (k unless the phase ended)."""
    T, d, base = phase1_state(A, b)
    out = dict.fromkeys(("done",) + _CENSUS_KEYS, 0)
    out["done"] = _replay(T, d, base, k, _count_census(out))[0]
    return out


def _tile_merges(v):
    """(the reference's pass 2, a left-to-right eps-scan, a right-to-left eps-scan) over the true
    512-element tile winners of v: the index each merge order picks"""
    pv, pi = [], []
    for t0 in range(0, len(v), 512):
        a, i = oracle.argmin_tile(v[t0:t0 + 512], t0)
        pv.append(a)
        pi.append(i)
    pv, pi = np.array(pv), np.array(pi, dtype=np.int64)
    rev = len(pv) - 1 - eps_scan(pv[::-1].copy())
    return oracle.argmin_pass2(pv, pi)[0], int(pi[eps_scan(pv)]), int(pi[rev])


def _count_merges(out):
    def count(v, e, rv, r):
        for side, vec, win in (("enter", v, e), ("ratio", rv, r)):
            ref, lin, rev = _tile_merges(vec)
            assert ref == win  # (tiles + pass 2 = the whole argmin below 1024 tiles)
            out[side + "_lin"] += lin != ref
            out[side + "_rev"] += rev != ref
    return count


def tile_merge_census(A, b, k):
    """Pivots (of k) at which merging the tile winners in another order than the reference's pass 2
    picks another index -- what a tile hand-off that combined records linearly, or ranks in another
    order, would get wrong: `*_lin` left to right, `*_rev` right to left; entering / ratio side."""
    T, d, base = phase1_state(A, b)
    out = dict.fromkeys(("done",) + _MERGE_KEYS, 0)
    out["done"] = _replay(T, d, base, k, _count_merges(out))[0]
    return out


def phase2_state(T, d, base, c):
    """phase 2's canonical state as the batch kernels (and orc_two_phase) set it up from phase 1's
    final one: the artificial columns leave d, d[1 : 1+n] = -c, the slack costs are zeroed, d[0] is
    kept, then update_objective at width 1 + n + m.  T is shared, d is new."""
    m, n = T.shape[0], len(c)
    d2 = d[:1 + n + m].copy()
    d2[1:1 + n] = -np.asarray(c, dtype=np.float64)
    d2[1 + n:] = 0.0
    oracle.update_objective(T, d2, base)
    return T, d2, base


def census_two_phase(A, b, c):
    """`census` and `tile_merge_census` over both phases of the whole solve of (A, b, c), which has
    to end FEASIBLE: {1: counts of phase 1, 2: counts of phase 2, "pivots": (p1, p2)}.  The replay's
    pivot counts and final basis are asserted equal to oracle.two_phase's."""
    ref = oracle.two_phase(A, b, c)
    assert ref["status"] == oracle.FEASIBLE
    m, n = A.shape
    out = {}
    T, d, base = phase1_state(A, b)
    for phase in (1, 2):
        cnt = dict.fromkeys(("done",) + _CENSUS_KEYS + _MERGE_KEYS, 0)
        a, t = _count_census(cnt), _count_merges(cnt)
        cnt["done"], st = _replay(T, d, base, -1, lambda *x: (a(*x), t(*x)))
        assert st == oracle.FEASIBLE
        out[phase] = cnt
        if phase == 1:
            assert not _negative(d[0]) and not np.any(base >= n + m)  # (phase 1 ended FEASIBLE)
            T, d, base = phase2_state(T, d, base, c)
    out["pivots"] = (out[1]["done"], out[2]["done"])
    assert out["pivots"] == ref["pivots"] and np.array_equal(base, ref["base"])
    return out


# ------------------------------------------------------------------ stand-in solvers
def select_np(vec):
    """a selection rule that is not the reference's: the plain minimum"""
    return int(np.argmin(vec))


def select_tiles_rev(vec):
    """a selection rule that is not the reference's: its tree inside every 512-wide tile, the tile
    winners merged right to left (more than 512 candidates only; below, the reference's rule)"""
    return _tile_merges(vec)[2] if len(vec) > 512 else oracle.argmin(vec)[0]


def _standin_solve(T, d, base, select, max_pivots):
    """orc_solve with `select` in place of the eps-argmin tree on both sides"""
    k = 0
    while True:
        if 0 <= max_pivots <= k:
            return oracle.PIVOT_CAP, k
        e = select(d[1:])
        dmin = d[1 + e]
        if not _negative(dmin):
            return oracle.FEASIBLE, k
        if not np.any(T[:, 1 + e] >= EPS):
            return oracle.UNBOUNDED, k
        r = select(ratios(T, e))
        base[r] = e
        prow, colE = T[r, :len(d)].copy(), T[:, 1 + e].copy()
        oracle.apply_update(T, d, prow, colE, r, prow[1 + e], dmin)
        k += 1


def standin_two_phase(A, b, c, select, max_pivots=-1):
    """orc_two_phase with `select` as the selection rule: what a batch kernel with that rule in
    place of wg_argmin's tree would return -- oracle.two_phase's fields plus the objective "row" """
    m, n = A.shape
    T, d, base = phase1_state(A, b)
    st, p1 = _standin_solve(T, d, base, select, max_pivots)
    p2 = 0
    if st != oracle.PIVOT_CAP:
        st = oracle.INFEASIBLE if _negative(d[0]) else \
            oracle.DEGENERATE if np.any((base >= n + m) & (base < n + 2 * m)) else oracle.FEASIBLE
    if st == oracle.FEASIBLE:
        T, d, base = phase2_state(T, d, base, c)
        st, p2 = _standin_solve(T, d, base, select, max_pivots)
    x, opt = np.zeros(n), 0.0
    if st == oracle.FEASIBLE:
        opt = float(d[0])
        x[base[base < n]] = T[base < n, 0]
    return {"status": st, "x": x, "opt": opt, "base": base, "pivots": (p1, p2), "row": d}


def same_result(got, ref):
    """every field the GPU tests compare (tests/batch_refs.py same_as_refs), as one boolean"""
    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    if got["status"] != ref["status"] or got["pivots"] != ref["pivots"] or not np.array_equal(got["base"], ref["base"]):
        return False
    if ref["status"] == oracle.FEASIBLE and not (np.array_equal(bits(got["opt"]), bits(ref["opt"]))
                                                 and np.array_equal(bits(got["x"]), bits(ref["x"]))):
        return False
    return len(got["row"]) == len(ref["row"]) and np.array_equal(bits(got["row"]), bits(ref["row"]))


# ------------------------------------------------------------------ first diverging pivot
def oracle_trace(T, d, base, k):
    """(pivots [(e, r)], basis after 0..done pivots, status, final (T, d, base)) on copies"""
    T, d, base = T.copy(), d.copy(), base.copy()
    piv, bases, st = [], [base.copy()], oracle.PIVOT_CAP
    for _ in range(k):
        s, e, r = oracle.pivot(T, d, base)
        if s != oracle.NOT_ENDED:
            st = s
            break
        piv.append((e, r))
        bases.append(base.copy())
    return piv, bases, st, (T, d, base)


def _window_text(vec, win, also):
    """the values within 2 eps of the oracle's winner, as offsets from it in units of eps"""
    near = np.flatnonzero(np.abs(vec - vec[win]) < 2 * EPS) if np.isfinite(vec[win]) else np.array([win])
    keep = sorted(set(near[:12].tolist()) | {win} | ({also} if also is not None and 0 <= also < len(vec) else set()))
    return ", ".join("%s[%d] %+.4f eps" % ("*" if i == win else "", i, (vec[i] - vec[win]) / EPS) for i in keep) + \
        " (%d values within 2 eps of the oracle's winner %r, marked *)" % (near.size, float(vec[win]))


def _bound(bases, got_base, got_done):
    """An upper bound on the first pivot the device chose differently, from its basis alone.  Each
    pivot rewrites one basis entry, so a device that agrees with the oracle through pivot j - 1 ends,
    after got_done pivots, at most got_done - j entries away from the oracle's basis after j pivots:
    the first j that breaks this lies past the first diverging pivot.  None: no j breaks it."""
    for j in range(1, len(bases)):
        if np.count_nonzero(got_base != bases[j]) > max(got_done - j, 0):
            return j - 1
    return None


def _forced_pivot(T, d, base, e, r):
    """one pivot with the entering column e and / or the leaving row r forced (None: the oracle's
    rule); False when no such pivot exists"""
    if e is None:
        e = oracle.argmin(d[1:])[0]
    if e < 0 or not d[1 + e] <= -EPS:
        return False
    if r is None:
        r = oracle.argmin(ratios(T, e))[0]
    if r < 0 or not T[r, 1 + e] >= EPS:
        return False
    base[r] = e
    prow, colE = T[r].copy(), T[:, 1 + e].copy()
    oracle.apply_update(T, d, prow, colE, r, prow[1 + e], d[1 + e])
    return True


def _lowest(v, cand, cap=12):
    """the `cap` candidates of lowest value (what another combine order would pick first)"""
    return cand[np.argsort(v[cand], kind="stable")][:cap]


def _single_fault(T0, d0, base0, piv, upto, got_base, got_done, budget_s=30.0):
    """CPU only: the first pivot j <= upto at which ONE different choice among the values within
    2 eps of the oracle's winner (entering or leaving), followed by the oracle's own rule, ends at
    the device's basis -- or None (several faults, or none of this kind)."""
    import time
    t0 = time.time()
    T, d, base = T0.copy(), d0.copy(), base0.copy()
    for j in range(min(upto, len(piv) - 1) + 1):
        e, r = piv[j]
        v, rv = d[1:], ratios(T, e)
        alts = [(int(a), None) for a in _lowest(v, np.flatnonzero(np.abs(v - v[e]) < 2 * EPS)) if a != e]
        if np.isfinite(rv[r]):
            alts += [(None, int(a)) for a in _lowest(rv, np.flatnonzero(np.abs(rv - rv[r]) < 2 * EPS)) if a != r]
        for ea, ra in alts:
            if time.time() - t0 > budget_s:
                return None
            T2, d2, b2 = T.copy(), d.copy(), base.copy()
            if not _forced_pivot(T2, d2, b2, ea, ra):
                continue
            done = j + 1 + oracle.solve(T2, d2, b2, max_pivots=got_done - j - 1)[1] if got_done > j + 1 else j + 1
            if done == got_done and np.array_equal(b2, got_base):
                return j
        oracle.pivot(T, d, base)
    return None


def explain_divergence(T0, d0, base0, k, got_base, got_done, run_device):
    """The text of a failed parity assertion: the first diverging pivot.

    The oracle is replayed pivot by pivot on the CPU.  The device's final basis bounds the first
    pivot it chose differently (_bound), and below that bound the CPU looks for the pivot at which a
    single different choice inside the winner's eps-window explains the device's basis
    (_single_fault).  One extra device run, `run_device(j + 1)` -> (T, d, base, status, done) from
    the initial state, at that pivot (else at the bound), shows the device's own choice at pivot j
    -- the one basis entry that differs from the oracle's basis after j pivots -- and the eps-window
    around the oracle's winner is printed.  When that run shows an earlier divergence, the bound is
    tightened from its basis on the CPU and reported as a bound."""
    piv, bases, st, _ = oracle_trace(T0, d0, base0, k)
    if not piv:
        return "the oracle takes no pivot (status %d)" % st
    j = _bound(bases, got_base, got_done)
    if j is None:
        if np.array_equal(got_base, bases[-1]) and got_done == len(piv):
            return "the device's basis equals the oracle's: the same pivots as far as the basis tells, different arithmetic"
        j = max(min(got_done, len(piv)) - 1, 0)
    j1 = _single_fault(T0, d0, base0, piv, j, got_base, got_done)
    j = j if j1 is None else j1
    Tg, dg, bg, sg, doneg = run_device(j + 1)
    msg = "first diverging pivot: %d (0-based) of %d, where the oracle enters %d and row %d leaves; " % (
        j, len(piv), piv[j][0], piv[j][1])
    if np.array_equal(bg, bases[j + 1]) and doneg == j + 1:
        return msg + "NOT CONFIRMED: run alone, the device agrees through pivot %d (a later pivot, or the batch " \
            "position, decides)" % j
    diff = np.flatnonzero(bg != bases[j])
    if doneg != j + 1 or diff.size != 1:
        j2 = _bound(bases[:j + 2], bg, doneg)
        return msg + "after %d pivots the device (done %d) differs from the oracle's basis after %d pivots in rows %s: " \
            "it diverged at or before pivot %s" % (j + 1, doneg, j, diff[:8].tolist(), j if j2 is None else j2)
    r_dev, e_dev = int(diff[0]), int(bg[diff[0]])
    T, d, base = T0.copy(), d0.copy(), base0.copy()
    for _ in range(j):
        oracle.pivot(T, d, base)
    e, r = piv[j]
    if e_dev != e:
        return msg + "the device ENTERS %d instead (row %d leaves); d[1:] around the oracle's winner: %s" % (
            e_dev, r_dev, _window_text(d[1:], e, e_dev))
    return msg + "the device's LEAVING row is %d instead (entering %d agrees); ratios around the oracle's winner: %s" % (
        r_dev, e, _window_text(ratios(T, e), r, r_dev))


# ------------------------------------------------------------------ first diverging pivot of a whole solve
def _first_bad(lo, hi, bad):
    """the smallest k in (lo, hi] with bad(k), given not bad(lo) and bad(hi): bisection"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bad(mid):
            hi = mid
        else:
            lo = mid
    return hi


def explain_batch_divergence(A, b, c, run_device):
    """The text of a failed whole-solve comparison of a batch entry: the first pivot count at which
    the device's basis is not the oracle's.  The batch entries take whole LPs only, so the device is
    probed through its pivot cap: `run_device(k)` -> (status, (p1, p2), base) of the solve with
    max_pivots = k.  A cap k <= p1 (the oracle's phase-1 count) stops in phase 1 after k pivots; a
    cap k > p1 lets phase 1 end and stops phase 2 after k pivots, so of phase 2 only the counts
    above p1 can be probed.  Bisection over phase 1, then over phase 2: about log2(p1) + log2(p2)
    device runs.  The eps-window around the oracle's winner at that pivot is printed."""
    m, n = A.shape
    T0, d0, base0 = phase1_state(A, b)
    piv1, bases1, st1, (T1, d1, base1) = oracle_trace(T0, d0, base0, 1 << 40)
    p1 = len(piv1)
    runs = []

    def bad(phase, bases):
        def f(k):
            st, piv, base = run_device(k)
            runs.append(k)
            want = (k, 0) if phase == 1 else (p1, k)
            return tuple(piv) != want or not np.array_equal(base, bases[k])
        return f

    def report(phase, k, T, d, base, piv, bases):
        # (T, d, base): the phase's initial state; the pivot that takes the count to k is piv[k - 1]
        st, pv, got = run_device(k)
        for _ in range(k - 1):
            oracle.pivot(T, d, base)
        e, r = piv[k - 1]
        msg = "first differing basis: after %d pivots of phase %d (device: status %d, pivots %r), where the oracle " \
            "enters %d and row %d leaves; " % (k, phase, st, tuple(pv), e, r)
        diff = np.flatnonzero(got != bases[k - 1])
        if diff.size != 1:
            return msg + "the device's basis differs from the oracle's basis after %d pivots in rows %s" % (
                k - 1, diff[:8].tolist())
        r_dev, e_dev = int(diff[0]), int(got[diff[0]])
        if e_dev != e:
            return msg + "the device ENTERS %d instead (row %d leaves); d[1:] around the oracle's winner: %s" % (
                e_dev, r_dev, _window_text(d[1:], e, e_dev))
        return msg + "the device's LEAVING row is %d instead (entering %d agrees); ratios around the oracle's winner: %s" % (
            r_dev, e, _window_text(ratios(T, e), r, r_dev))

    f1 = bad(1, bases1)
    if p1 and f1(p1):
        return report(1, _first_bad(0, p1, f1), T0, d0, base0, piv1, bases1) + " (device runs: %d)" % (len(runs) + 1)
    if st1 != oracle.FEASIBLE or _negative(d1[0]) or np.any(base1 >= n + m):
        return "the bases agree through phase 1 (%d pivots), which is where the oracle ends" % p1
    T2, d2, base2 = phase2_state(T1.copy(), d1, base1.copy(), c)
    piv2, bases2, _, _ = oracle_trace(T2, d2, base2, 1 << 40)
    p2 = len(piv2)
    f2 = bad(2, bases2)
    if p2 <= p1:
        return "the bases agree through phase 1 (%d pivots); phase 2 (%d pivots) is no longer than phase 1, so the " \
            "pivot cap cannot stop inside it" % (p1, p2)
    if not f2(p2):
        return "the bases agree through phase 1 (%d pivots) and after %d pivots of phase 2: the same pivots as far " \
            "as the basis tells, different arithmetic" % (p1, p2)
    if f2(p1 + 1):
        return "the bases agree through phase 1 (%d pivots) and differ after %d pivots of phase 2, the smallest count " \
            "the pivot cap can stop phase 2 at" % (p1, p1 + 1)
    return report(2, _first_bad(p1 + 1, p2, f2), T2, d2, base2, piv2, bases2) + " (device runs: %d)" % (len(runs) + 1)
