"""Dual ladders: kept batch states on which the order of the eps-argmin tree decides the kept-state
entries' own selections (sx_batch.hip wg_dual, wg_drop, k_batch_solve_cut).

tie_ladders.py pins the primal loop's two selections.  Six more wg_argmin call sites arrived with the
kept-state entries, each with its own lambda, length and scratch: the dual loop's entering ratio
d[1 + j] / -T[r][1 + j] and leaving row, the forced primal ratio of a dropped row (the slack moving up,
`forced+`, or on the negated column, `forced-`), the forced dual entering ratio of a dropped column (with
its `idx != v` exclusion and its `minus` sign), and the Gomory source row (key -min(f0, 1 - f0), rows
already taken marked).  All values below lie on the grid q = 0.125e-9 around 1.0 (1/2 for the cut keys),
so the candidates form eps-chains and the winner depends on the combine order: 32-lane shuffles, 512-wide
tiles, pass 2 over the tile winners.

  (a) origin()    the kept state is the raw [b | A | I]: the entering ratios are set through the costs and
                  the leaving ladder through b'.  The dual loop makes one pivot per ladder row.  The same
                  row through the rows entry (rows_case) has the new row's slack leaving.
  (b) k1_case()   the out-state K1 of (a) with one negative row: dropping the column x_e that entered is
                  the forced dual selection, the bound x_e <= 0.5 reaches the dual loop through the branch
                  front, both over a ladder whose every value lies within eps of every other.  minus_lp():
                  a phase-3 state in which x_e's row is negative, for the `minus` sign.
  (c) chain()     x_i - x_{i-1} <= q (k_i - k_{i-1}) below a bound on x_0: dropping that bound is a forced
                  primal ratio over the ladder x_i, `forced+` or `forced-`.
  (d) box()       x_j <= 3.5 + q k_j: every box row is an eligible source row with the key -(1/2 - q k_j).

Two row tiles: a chain or a box with L = 520 ladder rows needs n >= L and lies beyond the workspace class
(m (1 + n + m) doubles > 2^19), so the two-tile cases hold 300 ladder rows at random positions among 520
rows; the other rows are fillers that are never eligible.

`picks` is the census of one decision (the tree's pick against np.argmin, tie_ladders.eps_scan and, over
more than 512 candidates, tie_ladders.select_tiles_rev; `window`: the values inside the winner's
eps-window), `decided` the condition the pinned decisions meet: the tree differs from all of them.  A
stand-in is the restatement with another rule at one site (STANDINS through the reference helpers'
enter_argmin / leave_argmin / argmin keywords).  tests/test_dual_ladders.py holds every condition on the
CPU, tests/test_gpu_dual_ladders.py runs the cases through every kept-state entry.

Census of the (a) cases' dual loops through the rhs entry (committed seed; per side: candidates, pivots
`decided`, pivots where the tree differs from np.argmin / the eps-scan / the right-to-left tile merge):

    case    (n, m, groups, g)    seed class dual   enter: len dec arg scan rev | leave: len dec arg scan rev   floors
    A-1t    (120, 12, 4, 28)       2    2     4          132   2   3   3    -  |          12   1   1   1    -    2 / 1
    A-2t    (600, 4, 2, 280)       2    2     2          604   2   2   2    2  |           4   0   0   1    -    2 / 0
    A-3t    (1100, 12, 4, 250)     1    2     4         1112   2   3   3    4  |          12   2   2   2    -    2 / 2
    A-1024  (1012, 12, 4, 240)     7    2     4         1024   3   4   3    4  |          12   3   3   3    -    3 / 3
    A-1025  (1013, 12, 4, 240)     7    2     4         1025   3   4   3    4  |          12   1   1   1    -    3 / 1
    A-ws3   (1100, 24, 4, 250)     2    1     4         1124   3   4   3    4  |          24   1   1   1    -    3 / 1
    A-rows  (480, 520, 40, 12)     3    1    40         1000   0  32  23    0  |         520  15  31  26   28    0 / 12

The single pinned decisions (index each rule picks; window: values inside the winner's eps-window):

    pin                site         candidates  tree  argmin  scan  rev   window
    rows/A-1t          dual-enter      132        18      7      3      -     18
    rows/A-2t          dual-enter      604        20     38      1    512    207
    rows/A-3t          dual-enter     1112         8      4      4   1030    170
    rows/A-1024        dual-enter     1024       192     47     43    520    110
    rows/A-1025        dual-enter     1025       192     47     43    520     99
    rows/A-ws3         dual-enter     1124        20     15     13   1028    189
    drop/K-1t          forced-dual     132         6      7      3      -     25
    branch/K-1t        dual-enter      133         6      7      3      -     25
    drop/K-2t          forced-dual     604         2     38      1    512    142
    branch/K-2t        dual-enter      605         2     38      1    512    142
    drop/K-3t          forced-dual    1112       350     38      2   1024    105
    branch/K-3t        dual-enter     1113       350     38      2   1024    105
    drop/K-ws3         forced-dual    1124        12     73     33   1030    179
    branch/K-ws3       dual-enter     1125        12     73     33   1030    179
    drop-minus/M-1t    forced-dual     132        18      7      3      -     18
    drop-minus/M-3t    forced-dual    1112         8      4      4   1030    170
    drop/C+24          forced+          27        20      3      3      -      9
    drop/C-24          forced-          24        16      6      2      -     12
    drop/C+2t          forced+         520        24     20      5    512    199
    drop/C-2t          forced-         520        16      3      1    514    187
    drop2/C+24         forced+          27        20      3      3      -      9
    cut1/X-24          cut-row          24         0     22      7      -     20
    cut3/X-24          cut-row          24    0, 16, 8    22      7      -     20, 19, 20
    cut1/X-2t          cut-row         520        16    158      5    512    159
    cut3/X-2t          cut-row         520   16, 6, 17   158      5    512    159, 160, 240

In every row np.argmin at that site alone -- and, over more than 512 candidates, the right-to-left tile
merge -- ends at a result that fails the GPU file's comparison.
"""
import numpy as np

import oracle
import tie_ladders as tl
from batch_branch_refs import ref_branch
from batch_cut_refs import ref_cut
from batch_drop_refs import COLS, ROWS, ref_drop, reduced
from batch_rhs_refs import ref_rhs
from batch_rows_refs import ref_rows
from batch_state_refs import _once, bits, ref_state

Q = 0.125e-9
EPS = tl.EPS


# ------------------------------------------------------------------ selection rules as argmin(v) -> (index, value)
def _rule(select):
    def argmin(v):
        v = np.asarray(v, dtype=np.float64)
        i = int(select(v))
        return i, float(v[i])
    return argmin


np_rule = _rule(tl.select_np)            # the plain minimum
scan_rule = _rule(tl.eps_scan)           # a left-to-right eps-scan
rev_rule = _rule(tl.select_tiles_rev)    # the tree inside every tile, the tile winners merged right to left
STANDINS = {"np.argmin": np_rule, "tiles merged right to left": rev_rule}


class Recorder:
    """oracle.argmin that keeps every candidate vector it was given and what it picked"""

    def __init__(self):
        self.seen = []

    def __call__(self, v):
        v = np.array(v, dtype=np.float64)
        i, x = oracle.argmin(v)
        self.seen.append((v, i))
        return i, x


def picks(v, tree):
    """one decision's census: what the other rules pick, and the winner's eps-window"""
    return {"len": len(v), "tree": tree, "argmin": tl.select_np(v), "scan": tl.eps_scan(v),
            "rev": tl.select_tiles_rev(v) if len(v) > 512 else None, "window": int(tl.window(v, tree).size)}


def decided(p):
    """the tree's pick differs from np.argmin's and from the eps-scan's -- and, over more than one
    tile, from the right-to-left tile merge's"""
    return p["tree"] != p["argmin"] and p["tree"] != p["scan"] and (p["rev"] is None or p["tree"] != p["rev"])


# ------------------------------------------------------------------ (a) origin LPs
def origin(n, m, groups, g, seed, levels=16):
    """(A, b, c, b', ladder rows, [columns of group t]): phase 1 is m slack pivots on 1.0 and phase 2
    takes none, so the kept state is [b | A | I] with d[1 : 1 + n] = -c = 1 + q k_j.  Ladder row r_t
    holds -1.0 on its own group of g columns, which are zero in every other row; b' is b with
    b'[r_t] = -(1 + 2 q k'_t)"""
    rng = np.random.default_rng(seed)
    assert groups * g <= n and groups <= m
    c = -(1.0 + Q * rng.integers(0, levels, size=n))
    b = rng.integers(1, 9, size=m).astype(np.float64)
    A = rng.integers(0, 6, size=(m, n)) / 128.0 if m <= 20 else (rng.random((m, n)) < 8.0 / m) / 128.0
    rows = np.sort(rng.permutation(m)[:groups])
    perm = rng.permutation(n)
    cols = [np.sort(perm[t * g:(t + 1) * g]) for t in range(groups)]
    A[rows, :] = 0.0
    for t in range(groups):
        A[:, cols[t]] = 0.0
        A[rows[t], cols[t]] = -1.0
    b2 = b.copy()
    b2[rows] = -(1.0 + 2 * Q * rng.integers(0, levels, size=groups))
    return np.ascontiguousarray(A), b, c, b2, rows, cols


def is_raw(state, A, b, c):
    """the kept state is [b | A | I] bit for bit, after (m, 0) pivots, with d = 0 | -c | 0"""
    m, n = A.shape
    T = np.concatenate([b[:, None], A, np.eye(m)], axis=1)
    d = np.zeros(1 + n + 2 * m)
    d[1:1 + n] = -c
    return (state["status"] == oracle.FEASIBLE and state["pivots"] == (m, 0) and state["phase"] == 2
            and np.array_equal(bits(state["T"]), bits(T)) and np.array_equal(bits(state["d"]), bits(d))
            and np.array_equal(state["base"], n + np.arange(m)))


# ------------------------------------------------------------------ (c) chain LPs
def chain(L, m, sign, seed, levels=16):
    """(A [m, L + 1], b, c, pos, k): x_0 is bounded by row pos[0] -- from above (sign +1: x_0 <= 1 + q k_0) or from
    below (sign -1: -x_0 <= -(1 + q k_0), c_0 = -(L + 1)) --, x_i - x_{i-1} <= q (k_i - k_{i-1}) and
    c_i = 1, so every chain row is tight, x is the ladder 1 + q k_i and slack 0 is nonbasic with sign
    in all L chain rows.  Chain row i stands at pos[i], random positions among m - L filler rows
    y <= 5 on a variable of their own (cost -1: y stays nonbasic, the filler slacks basic, slack 0's
    entries there 0); with sign +1 the first filler row is sum x <= 4 L instead, which keeps the LP
    bounded without the row of x_0 (that slack's entry there: -L)"""
    rng = np.random.default_rng(seed)
    assert sign in (1, -1) and m >= L + (1 if sign > 0 else 0)
    k = rng.integers(0, levels, size=L)
    n = L + 1
    A, b = np.zeros((m, n)), np.full(m, 5.0)
    A[:, L] = 1.0
    pos = np.sort(rng.permutation(m)[:L])
    A[pos, L] = 0.0
    A[pos[0], 0], b[pos[0]] = sign, sign * (1.0 + Q * k[0])
    for i in range(1, L):
        A[pos[i], i], A[pos[i], i - 1], b[pos[i]] = 1.0, -1.0, Q * (int(k[i]) - int(k[i - 1]))
    c = np.ones(n)
    c[L] = -1.0
    if sign > 0:
        r = next(i for i in range(m) if i not in set(pos.tolist())) if m > L else None
        A[r, :L], A[r, L], b[r] = 1.0, 0.0, 4.0 * L
    else:
        c[0] = -(L + 1.0)
    return np.ascontiguousarray(A), b, c, pos, k


# ------------------------------------------------------------------ (d) box LPs
def box(L, m, seed, levels=16):
    """(A [m, L + 2], b, c): x_j <= 3.5 + q k_j with c_j = 1, so x_j is basic in its own row at a value
    whose fractional part is 1/2 + q k_j: the key of that row is -(1/2 - q k_j).  Two more columns with
    cost -1 and entries in {1/4, 1/2, 3/4} make the cuts dense.  The box rows stand at random positions
    among m - L filler rows on the two extra columns alone, whose slacks stay basic"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, levels, size=L)
    n = L + 2
    A = np.zeros((m, n))
    A[:, L:] = rng.integers(1, 4, size=(m, 2)) / 4.0
    b = np.full(m, 5.0)
    pos = np.sort(rng.permutation(m)[:L])
    A[pos, np.arange(L)] = 1.0
    b[pos] = 3.5 + Q * k
    c = np.ones(n)
    c[L:] = -1.0
    return np.ascontiguousarray(A), b, c, pos, k


def minus_lp(n, m, g, seed, levels=16):
    """(A, b, c, b', p, e): an origin LP with two groups and one more column e, +1.0 in row p = the
    ladder row of group 0 and zero elsewhere, with the only positive cost, 1/2.  x_e enters the basis
    on that 1.0 (its column sum ties with the slacks' in phase 1), after which it is basic in row p --
    which still holds -1.0 on group 0 -- and d_j = 1/2 + q k_j there.
    b' makes row p negative (-1/4) and the ladder row of group 1 more negative,
    so a re-solve capped at one dual pivot leaves a phase-3 state in which x_e's row has a negative
    right-hand side: dropping column e is the forced dual selection with `minus`"""
    A, b, c, b2, rows, cols = origin(n, m, 2, g, seed, levels)
    p = int(rows[0])
    e = int(np.setdiff1d(np.arange(n), np.concatenate(cols))[0])
    A[:, e] = 0.0
    A[p, e] = 1.0
    c[e] = 0.5
    b2[p] = -0.25
    return A, b, c, b2, p, e


# ------------------------------------------------------------------ the committed cases
# (a): name -> ((n, m, groups, g), seed, batch class, floor of dual pivots the tree decides on the
# entering side, on the leaving side).  A floor is a condition on the input: a seed that misses it is
# replaced, the floor stays.
ORIGIN = {
    "A-1t": ((120, 12, 4, 28), 2, 2, 2, 1),        # 132 candidates: the lane tree
    "A-2t": ((600, 4, 2, 280), 2, 2, 2, 0),        # 604 candidates, two tiles
    "A-3t": ((1100, 12, 4, 250), 1, 2, 2, 2),      # three tiles, the last one partial
    "A-1024": ((1012, 12, 4, 240), 7, 2, 3, 3),    # n + m = 1024: exactly two full tiles
    "A-1025": ((1013, 12, 4, 240), 7, 2, 3, 1),    # 1025 candidates: the third tile holds one value
    "A-ws3": ((1100, 24, 4, 250), 2, 1, 3, 1),     # three tiles in the workspace class
    "A-rows": ((480, 520, 40, 12), 3, 1, 0, 12),   # the leaving ladder (40 rows) over two row tiles
}


def neighbours(cls):
    """a case rides with its seed neighbours: 3 problems in the LDS class, 2 in the workspace class"""
    return 3 if cls == 2 else 2


def origin_case(name, seed=None):
    """a committed (a) case, or its neighbour of another seed: the instance, b', its ladder rows and
    groups, and the kept state; computed once, do not write it"""
    shape, seed0 = ORIGIN[name][:2]
    seed = seed0 if seed is None else seed

    def make():
        A, b, c, b2, rows, cols = origin(*shape, seed)
        return {"A": A, "b": b, "c": c, "b2": b2, "rows": rows, "cols": cols, "state": ref_state(A, b, c)}
    return _once(("dl-origin", name, seed), make)


def want_rhs(case, max_pivots=-1, **sel):
    """the re-solve of the kept state for b' (sel: ref_rhs's selections)"""
    return ref_rhs(case["state"], case["A"], case["b2"], case["c"], max_pivots, **sel)


def rows_case(case):
    """the same entering ladder through the rows entry: the instance without ladder row r_0, its kept
    state, and the grown problem with the row -sum_{group 0} x_j <= -1 appended"""
    r0 = int(case["rows"][0])
    A0, b0 = np.ascontiguousarray(np.delete(case["A"], r0, axis=0)), np.delete(case["b"], r0)
    row = np.zeros(A0.shape[1])
    row[case["cols"][0]] = -1.0
    return {"A0": A0, "b0": b0, "c": case["c"], "A": np.ascontiguousarray(np.vstack([A0, row])),
            "b": np.append(b0, -1.0), "state": ref_state(A0, b0, case["c"])}


def want_rows(rc, max_pivots=-1, **sel):
    return ref_rows(rc["state"], rc["A"], rc["b"], rc["c"], max_pivots, **sel)


def k1_case(case):
    """(b): the out-state K1 of a re-solve that makes only b'[r_0] negative: one structural x_e of
    group 0 is basic in row r_0 at 1.0, the row holds +1.0 on the rest of the group, and every d_j there
    is q (k_j - k_e)"""
    r0 = int(case["rows"][0])
    b1 = case["b"].copy()
    b1[r0] = case["b2"][r0]
    K1 = ref_rhs(case["state"], case["A"], b1, case["c"])
    return {"A": case["A"], "b": b1, "c": case["c"], "state": K1, "e": int(K1["base"][r0]), "row": r0}


# (b): name -> (the (a) case whose shape it has, seed): the second step from that case's K1
SECOND = {"K-1t": ("A-1t", 2), "K-2t": ("A-2t", 2), "K-3t": ("A-3t", 2), "K-ws3": ("A-ws3", 1)}


def second_case(name, seed=None):
    a, seed0 = SECOND[name]
    return k1_case(origin_case(a, seed0 if seed is None else seed))


def want_drop_col(kc, max_pivots=-1, **sel):
    """drop_cols(K1, [e]): the forced dual entering selection"""
    return ref_drop(kc["state"], COLS, [kc["e"]], *reduced((kc["A"], kc["b"], kc["c"]), COLS, [kc["e"]]), max_pivots, **sel)


CHILDREN = ((1.0, 0.5), (-1.0, -1.5))  # x_e <= 0.5 and -x_e <= -1.5


def want_child(kc, child, max_pivots=-1, **sel):
    """a child of K1: the bound row on x_e through the branch front, then the dual loop"""
    coef, rhs = CHILDREN[child]
    return ref_branch(kc["state"], (kc["A"], kc["b"], kc["c"]), [kc["e"]], [coef], [rhs], max_pivots, **sel)


# the `minus` variant of the forced dual selection: name -> ((n, m, g), seed, class)
MINUS = {
    "M-1t": ((120, 12, 28), 2, 2),
    "M-3t": ((1100, 12, 250), 1, 2),
}


def minus_case(name, seed=None):
    """the phase-3 state a re-solve capped at one dual pivot leaves, in which x_e's row is negative"""
    shape, seed0 = MINUS[name][:2]
    seed = seed0 if seed is None else seed

    def make():
        A, b, c, b2, p, e = minus_lp(*shape, seed)
        st = ref_state(A, b, c)
        K = ref_rhs(st, A, b2, c, 1)
        return {"A": A, "b": b2, "c": c, "b0": b, "first": st, "state": K, "e": e, "row": p}
    return _once(("dl-minus", name, seed), make)


# (c): name -> ((L, m, sign), seed, class): drop the row of x_0
CHAIN = {
    "C+24": ((24, 27, 1), 5, 2),
    "C-24": ((24, 24, -1), 8, 2),
    "C+2t": ((300, 520, 1), 5, 1),    # 300 ladder rows among 520: two row tiles
    "C-2t": ((300, 520, -1), 1, 1),
}


def chain_case(name, seed=None, q=1):
    """the chain LP, its kept state, and the rows to drop: q = 1 the row of x_0, q = 2 also the row
    x_1 - x_0 <= ., which goes first (drops are applied in descending order)"""
    shape, seed0 = CHAIN[name][:2]
    seed = seed0 if seed is None else seed

    def make():
        A, b, c, pos, k = chain(*shape, seed)
        return {"A": A, "b": b, "c": c, "pos": pos, "k": k, "state": ref_state(A, b, c)}
    case = dict(_once(("dl-chain", name, seed), make))
    case["idx"] = sorted(int(r) for r in case["pos"][:q])
    return case


def want_drop_rows(cc, max_pivots=-1, **sel):
    return ref_drop(cc["state"], ROWS, cc["idx"], *reduced((cc["A"], cc["b"], cc["c"]), ROWS, cc["idx"]), max_pivots, **sel)


# (d): name -> ((L, m), seed, class of the shape grown by three cuts)
BOX = {
    "X-24": ((24, 24), 4, 2),
    "X-2t": ((300, 520), 2, 1),       # 300 eligible rows among 520: two row tiles
}


def box_case(name, seed=None):
    shape, seed0 = BOX[name][:2]
    seed = seed0 if seed is None else seed

    def make():
        A, b, c, pos, k = box(*shape, seed)
        return {"A": A, "b": b, "c": c, "pos": pos, "k": k, "state": ref_state(A, b, c)}
    return _once(("dl-box", name, seed), make)


def want_cut(xc, cuts, max_pivots=-1, **sel):
    """(cut_A, cut_b, cut_rows, the re-solve of the grown problem): all variables integer"""
    n = xc["A"].shape[1]
    return ref_cut(xc["state"], xc["A"], xc["b"], xc["c"], np.ones(n, dtype=bool), cuts, max_pivots=max_pivots, **sel)


# ------------------------------------------------------------------ comparisons
def same_result(got, want):
    """tie_ladders.same_result -- the fields the GPU tests compare through same_as_state_refs -- extended
    by the saved state (T, d, phase) and, for the cut entry's tuples, by cut_A, cut_b and cut_rows"""
    if isinstance(want, tuple):
        return (np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
                and np.array_equal(got[2], want[2]) and same_result(got[3], want[3]))
    return (tl.same_result(got, want) and got["phase"] == want["phase"] and got["T"].shape == want["T"].shape
            and np.array_equal(bits(got["T"]), bits(want["T"])) and np.array_equal(bits(got["d"]), bits(want["d"])))


def as_out(res):
    """a restatement's dict dressed as the BatchTensors a kept-state call returns (host tensors), so that
    the GPU file's own comparison, batch_state_refs.same_as_state_refs, can be held against it"""
    from types import SimpleNamespace

    import torch

    m, Ns = res["T"].shape
    row = np.zeros(Ns + m)
    row[:len(res["row"])] = res["row"]
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)[None].copy())  # noqa: E731
    state = SimpleNamespace(n=Ns - 1 - m, m=m, T=t(res["T"], np.float64), d=t(res["d"], np.float64),
                            base=t(res["base"], np.int32), phase=t(res["phase"], np.int32),
                            pivots=t(res["pivots"], np.int64))
    return SimpleNamespace(status=t(res["status"], np.int32), pivots=t(res["pivots"], np.int64),
                           optimal_value=t(res["opt"], np.float64), solution=t(res["x"], np.float64),
                           base=t(res["base"], np.int32), objective_row=t(row, np.float64),
                           row_width=t(len(res["row"]), np.int32), state=state)


def passes_the_gpu_comparison(got, want):
    """same_as_state_refs -- what tests/test_gpu_dual_ladders.py asserts of a call -- with the restatement
    `got` in the device's place; the cut entry's tuples also through cut_A, cut_b and cut_rows, as there"""
    from batch_state_refs import same_as_state_refs

    if isinstance(want, tuple):
        if not (np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
                and np.array_equal(got[2], want[2])):
            return False
        got, want = got[3], want[3]
    m, Ns = want["T"].shape
    if got["T"].shape != want["T"].shape:
        return False
    try:
        same_as_state_refs(as_out(got), [want], Ns - 1 - m, m)
    except AssertionError:
        return False
    return True


def recorded(want, site, **kw):
    """the census of every decision the restatement `want(**kw, site=Recorder)` takes at `site` (a
    keyword of the reference helpers: enter_argmin, leave_argmin or argmin): [picks]"""
    rec = Recorder()
    want(**kw, **{site: rec})
    return [picks(v, i) for v, i in rec.seen]


def standin_results(want, site, **kw):
    """{rule name: the restatement with that rule at `site` alone}; the right-to-left tile merge only
    where the site has more than one tile"""
    tiles = any(p["len"] > 512 for p in recorded(want, site, **kw))
    return {name: want(**kw, **{site: rule}) for name, rule in STANDINS.items() if tiles or rule is not rev_rule}


# ------------------------------------------------------------------ the pinned decisions
SITES = ("dual-enter", "dual-leave", "forced+", "forced-", "forced-dual", "cut-row")


def pins():
    """every single decision the committed cases pin, beside the (a) cases' dual loops (ORIGIN's floors):
    [(id, site, the reference helpers' keyword of that site, want(**selections), decisions pinned,
    (n, m) of the launch's class, class)]"""
    from functools import partial

    out = []
    for name, (shape, _, cls, fe, _) in ORIGIN.items():
        if fe:
            out.append(("rows/" + name, "dual-enter", "enter_argmin", partial(want_rows, rows_case(origin_case(name))), 1,
                        shape[:2], cls))
    for name, (a, _) in SECOND.items():
        shape, cls = ORIGIN[a][0], ORIGIN[a][2]
        kc = second_case(name)
        out.append(("drop/" + name, "forced-dual", "argmin", partial(want_drop_col, kc), 1, shape[:2], cls))
        out.append(("branch/" + name, "dual-enter", "enter_argmin", partial(want_child, kc, 0), 1,
                    (shape[0], shape[1] + 1), cls))
    for name, ((n, m, _), _, cls) in MINUS.items():
        out.append(("drop-minus/" + name, "forced-dual", "argmin", partial(want_drop_col, minus_case(name)), 1, (n, m), cls))
    for name, ((L, m, sign), _, cls) in CHAIN.items():
        out.append(("drop/" + name, "forced+" if sign > 0 else "forced-", "argmin",
                    partial(want_drop_rows, chain_case(name)), 1, (L + 1, m), cls))
    out.append(("drop2/C+24", "forced+", "argmin", partial(want_drop_rows, chain_case("C+24", q=2)), 1, (25, 27), 2))
    for name, ((L, m), _, cls) in BOX.items():
        for cuts in (1, 3):
            out.append(("cut%d/%s" % (cuts, name), "cut-row", "argmin", partial(want_cut, box_case(name), cuts), cuts,
                        (L + 2, m + cuts), cls))
    return out
