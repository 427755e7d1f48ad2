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


# ------------------------------------------------------------------ the plain rules
def ratios(T, e):
    """createIndicatorsVector: b_i / a_ie where a_ie >= 1e-9, else DBL_MAX"""
    col = T[:, 1 + e]
    ok = col >= EPS
    out = np.full(T.shape[0], DBL_MAX)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        out[ok] = T[ok, 0] / col[ok]
    return out


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


def census(A, b, k):
    """Replay k pivots of (A, b)'s phase 1 with oracle.pivot and count the pivots the combine tree
    decides.  Per side (entering: d[1:]; ratio: the ratio vector of the entering column):
    `*_argmin` / `*_scan`: the oracle's choice differs from np.argmin / from eps_scan;
    `*_sensitive`: from either; `*_window`: the winner has a second, different value inside its
    eps-window.  `done`: pivots taken (k unless the phase ended)."""
    T, d, base = phase1_state(A, b)
    out = {"done": 0, "enter_argmin": 0, "enter_scan": 0, "enter_sensitive": 0, "enter_window": 0,
           "ratio_argmin": 0, "ratio_scan": 0, "ratio_sensitive": 0, "ratio_window": 0}
    for _ in range(k):
        v = d[1:].copy()
        e_pred = oracle.argmin(v)[0]
        rv = ratios(T, e_pred) if e_pred >= 0 else None
        st, e, r = oracle.pivot(T, d, base)
        if st != oracle.NOT_ENDED:
            break
        assert e == e_pred and r == oracle.argmin(rv)[0]
        out["done"] += 1
        for side, vec, win in (("enter", v, e), ("ratio", rv, r)):
            a, s = int(np.argmin(vec)) != win, eps_scan(vec) != win
            out[side + "_argmin"] += a
            out[side + "_scan"] += s
            out[side + "_sensitive"] += a or s
            out[side + "_window"] += window(vec, win).size > 0
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


def tile_merge_census(A, b, k):
    """Pivots (of k) at which merging the tile winners in another order than the reference's pass 2
    picks another index -- what a tile hand-off that combined records linearly, or ranks in another
    order, would get wrong: `*_lin` left to right, `*_rev` right to left; entering / ratio side."""
    T, d, base = phase1_state(A, b)
    out = {"done": 0, "enter_lin": 0, "enter_rev": 0, "ratio_lin": 0, "ratio_rev": 0}
    for _ in range(k):
        v = d[1:].copy()
        e = oracle.argmin(v)[0]
        rv = ratios(T, e) if e >= 0 else None
        if oracle.pivot(T, d, base)[0] != oracle.NOT_ENDED:
            break
        out["done"] += 1
        for side, vec in (("enter", v), ("ratio", rv)):
            ref, lin, rev = _tile_merges(vec)
            assert ref == oracle.argmin(vec)[0]  # (tiles + pass 2 = the whole argmin below 1024 tiles)
            out[side + "_lin"] += lin != ref
            out[side + "_rev"] += rev != ref
    return out


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
