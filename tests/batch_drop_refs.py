"""Constraint rows or structural columns taken out of a kept batch state (simplex_solve_batch_device_drop)
restated from the oracle's pieces -- argmin, ratio, the pivot of apply_update as batch_rhs_refs' dual loop
uses it -- and batch_rhs_refs (_enter_dual, dual_feasible), batch_state_refs (_run, ref_state), and nothing
else, for test_batch_drop_host.py (the oracle alone) and test_gpu_batch_drop.py (bit for bit against the
GPU).

The drops are applied one at a time in descending index order, each at the shape the earlier ones left:
np.delete after every drop, so oracle.argmin sees the current shape's positions and lengths.

A reference state is batch_state_refs' dict (phase 3 as in batch_rhs_refs), in the reduced shape.  A
result also says which path each drop took, in the order they were applied ("paths": none, forced+,
forced-, forced-dual), why the problem went cold ("why": None, phase-1, phase-3, dual-infeasible,
no-candidate) and both folded into one word ("path": cold, else the first forced path, else none).
"""
import numpy as np

import oracle
import simplexoncuda_amd as sx
from batch_cols_refs import append_column
from batch_rhs_refs import DBL_MAX, _enter_dual, dual_feasible
from batch_rows_refs import grow
from batch_state_refs import EPS, _negative, _once, _run, mixed_instances, ref_state

ROWS, COLS = 0, 1


def _pivot(T, d, base, r, e):
    """row r leaves, variable e enters: batch_rhs_refs._dual's pivot, d at the tableau's width"""
    prow, colE = T[r].copy(), T[:, 1 + e].copy()
    oracle.apply_update(T, d, prow, colE, r, prow[1 + e], d[1 + e])
    base[r] = e


def _basic_row(base, v):
    rows = np.flatnonzero(base == v)
    return int(rows[0]) if len(rows) else -1


def _without(T, d, base, row, col, v):
    """tableau row `row` (None: none) and stored column `col` deleted; basis entries above v go down by one"""
    if row is not None:
        T, base = np.delete(T, row, axis=0), np.delete(base, row)
    T, d = np.ascontiguousarray(np.delete(T, col, axis=1)), np.delete(d, col)
    return T, d, np.where(base > v, base - 1, base).astype(np.int32)


def ref_drop(state, kind, idx, A, b, c, max_pivots=-1, argmin=oracle.argmin):
    """the reduced state and results of `state` (left as it is) with the rows (kind ROWS) or columns (kind
    COLS) idx -- strictly ascending -- taken out; A [m, n], b [m], c [n] are the reduced problem; argmin: the
    selection of a forced pivot (the primal ratio of ROWS, the dual entering ratio of COLS), the oracle's
    eps-argmin tree unless a test swaps it"""
    m0, Ns0 = state["T"].shape
    n0 = Ns0 - 1 - m0
    idx = [int(v) for v in idx]
    q = len(idx)
    assert q >= 1 and all(x < y for x, y in zip(idx, idx[1:])) and 0 <= idx[0] and idx[-1] < (m0 if kind == ROWS else n0)
    assert A.shape == ((m0 - q, n0) if kind == ROWS else (m0, n0 - q))
    paths, why, forced = [], None, 0
    if state["phase"] == 1:
        why = "phase-1"
    else:
        basic = sum(_basic_row(state["base"], n0 + v if kind == ROWS else v) >= 0 for v in idx)
        if kind == ROWS and state["phase"] == 3 and basic != q:
            why = "phase-3"  # a forced primal pivot needs a primal feasible column
        elif kind == COLS and basic > 0 and not dual_feasible(state):
            why = "dual-infeasible"  # a forced dual pivot needs a dual feasible row
    if why is None:
        T, d, base = state["T"].copy(), state["d"][:Ns0].copy(), state["base"].copy()
        n, m = n0, m0
        for t in reversed(idx):
            v = n + t if kind == ROWS else t
            r = _basic_row(base, v)
            if kind == ROWS:
                if r >= 0:
                    paths.append("none")
                else:
                    col = T[:, 1 + v].copy()
                    if (col >= EPS).any():
                        a, path = col, "forced+"
                    elif (-col >= EPS).any():
                        a, path = -col, "forced-"  # the slack moves down; the pivot element is negative
                    else:
                        why = "no-candidate"
                        break
                    r, _ = argmin(np.array([oracle.ratio(T[i, 0], a[i]) for i in range(m)]))
                    if r < 0 or r >= m:
                        why = "no-candidate"
                        break
                    _pivot(T, d, base, r, v)
                    forced += 1
                    paths.append(path)
                T, d, base = _without(T, d, base, r, 1 + v, v)
                m -= 1
            else:
                if r < 0:
                    paths.append("none")
                else:
                    a = -T[r, 1:] if _negative(T[r, 0]) else T[r, 1:].copy()
                    elig = a >= EPS
                    elig[v] = False
                    if not elig.any():
                        why = "no-candidate"
                        break
                    e, _ = argmin(np.array([DBL_MAX if j == v else oracle.ratio(d[1 + j], a[j])
                                            for j in range(n + m)]))
                    if e < 0 or e >= n + m:
                        why = "no-candidate"
                        break
                    _pivot(T, d, base, r, e)
                    forced += 1
                    paths.append("forced-dual")
                T, d, base = _without(T, d, base, None, 1 + v, v)
                n -= 1
    if why is None:
        full = np.zeros(1 + n + 2 * m)
        full[:1 + n + m] = d
        first = (state["pivots"][0], forced)
        if state["phase"] == 3 or (kind == COLS and forced > 0):
            res = _enter_dual(T, full, base, first, c, max_pivots, oracle.argmin)
        else:
            res = _run(T, full, base, 2, first, c, max_pivots, False)
    else:
        res = dict(ref_state(A, b, c, max_pivots))  # (its arrays are shared: do not write them)
    res["paths"], res["why"], res["forced"] = paths, why, forced
    res["path"] = "cold" if why else next((p for p in paths if p != "none"), "none")
    return res


# ---- the instances both test files use ----
def reduced(inst, kind, idx):
    """the instance with the rows or columns idx deleted"""
    A, b, c = inst
    idx = list(idx)
    if kind == ROWS:
        return np.ascontiguousarray(np.delete(A, idx, axis=0)), np.delete(b, idx), c
    return np.ascontiguousarray(np.delete(A, idx, axis=1)), b, np.delete(c, idx)


def rows_shapes():
    """(n, m_in, q): smallest, small, q = 3, two mid shapes, the class edge, workspace in and LDS out (at
    n = 241 the LDS class ends behind m = 63), workspace to workspace, the forced ratio over two row tiles
    and the reduced one over one, the entering selection over two tiles"""
    return [(1, 2, 1), (5, 5, 1), (5, 7, 3), (20, 11, 1), (33, 32, 1), (64, 64, 1), (241, 64, 1), (241, 65, 1), (4, 513, 1),
            (600, 5, 1)]


def cols_shapes():
    """(n_in, m, q): as rows_shapes; (513 -> 512, 4) and (512 -> 511, 4) put the forced dual selection's
    1 + n + m - 1 candidates on either side of the first entering tile's edge"""
    return [(2, 1, 1), (6, 4, 1), (8, 4, 3), (21, 10, 1), (34, 31, 1), (64, 64, 1), (241, 64, 1), (242, 64, 1), (5, 513, 1),
            (513, 4, 1), (512, 4, 1), (600, 4, 1)]


def shapes(kind):
    return rows_shapes() if kind == ROWS else cols_shapes()


def drop_instances(n, m):
    """three generated instances in [1, 100] of the in-state's shape"""
    return _once(("drop", n, m), lambda: [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2, 3)])


def candidates(st, kind):
    """(indices that leave without arithmetic, indices that need a forced pivot) of a FEASIBLE phase-2
    state: rows by their slack basic or not; columns nonbasic, or basic with a positive value"""
    m, Ns = st["T"].shape
    n = Ns - 1 - m
    if kind == ROWS:
        free = [r for r in range(m) if (st["base"] == n + r).any()]
        return free, [r for r in range(m) if r not in free]
    held = {int(st["base"][i]): st["T"][i, 0] for i in range(m) if st["base"][i] < n}
    return [j for j in range(n) if j not in held], [j for j, v in held.items() if v >= EPS]


def choose(st, kind, q, k):
    """the list instance k of a batch drops: instance 0 only what leaves without arithmetic, instance 1
    only what needs a forced pivot (q = 1: the first such index), instance 2 the last such index, and for
    q > 1 both sorts mixed in one list; where a sort runs out the other fills the list"""
    free, tight = candidates(st, kind)
    if k == 0:
        pick = (free + tight)[:q]
    elif k == 1 or q == 1:
        pick = (tight + free)[:q] if k == 1 else (tight[::-1] + free)[:q]
    else:
        pick = (tight[-1:] + free[:q - 1] + tight[:-1] + free[q - 1:])[:q]
    return sorted(pick)


def want_batch(kind, n_in, m_in, q, max_pivots=-1):
    """a shape's three instances, their kept states, the lists, the reduced instances and what the drop
    must give, computed once: (insts, [ref_state], [idx], [reduced], [ref_drop]); do not write them"""
    def make():
        insts = list(drop_instances(n_in, m_in))
        refs = [ref_state(*inst) for inst in insts]
        if kind == ROWS and not candidates(refs[0], kind)[0]:
            # every row is tight (n far above m): the first instance gets a loose cut as its last row
            insts[0] = added_row(oracle.generate(n_in, m_in - 1, 1000 + n_in * 100 + m_in - 1, 1, 100), 1.5)
            refs[0] = ref_state(*insts[0])
        lists = [choose(st, kind, q, k) for k, st in enumerate(refs)]
        small = [reduced(inst, kind, idx) for inst, idx in zip(insts, lists)]
        return insts, refs, lists, small, [ref_drop(st, kind, idx, *g, max_pivots)
                                           for st, idx, g in zip(refs, lists, small)]
    return _once(("drop-want", kind, n_in, m_in, q, max_pivots), make)


def forced_minus_instance():
    """the optimum (4, 5) has row 0 tight and slack 0's column is (-1, 0): the slack can only move down"""
    return np.array([[-1.0, 1.0], [0.0, 1.0]]), np.array([1.0, 5.0]), np.array([-0.5, 1.0])


def handmade(kind):
    """(state, idx, reduced instance) of a forced selection without a candidate, hand-made from the kept
    state of the first (5, 5) / (6, 4) instance (T and d belong to the basis: the caller's contract):
    ROWS a tight row's slack column within eps of zero; COLS a basic column whose row holds nothing but
    its own unit entry"""
    n, m = (5, 5) if kind == ROWS else (6, 4)
    inst = drop_instances(n, m)[0]
    st = dict(ref_state(*inst))
    st["T"] = st["T"].copy()
    v = candidates(st, kind)[1][0]
    if kind == ROWS:
        st["T"][:, 1 + n + v] = [1e-12 * (-1) ** i for i in range(m)]
    else:
        i = int(np.flatnonzero(st["base"] == v)[0])
        st["T"][i, 1:] = 0.0
        st["T"][i, 1 + v] = 1.0
    return st, [v], reduced(inst, kind, [v])


ROUND_TRIP_SHAPES = [(32, 16), (64, 64)]  # the kept shape (n, m) a row or a column is added to and dropped from
CAP_ROWS, CAP_COLS = (241, 64, 1), (64, 64, 1)
DROP_CAPS = [1, 2, 8]
MIXED_SHAPE = (12, 10, 1)


def added_row(inst, theta):
    """the instance with one cut appended (batch_rows_refs.grow: theta < 1 binding, theta > 1 loose)"""
    return grow(inst, ["cut"], theta)


def added_col(inst, theta, seed=900):
    """the instance with one generated column appended, its cost scaled by theta (batch_cols_refs)"""
    return append_column(inst, seed, theta)


def needing_column_0(inst):
    """the instance with b scaled by 100 and the row -x_0 <= -1 appended: x_0 = 1 fits every row (A is at
    most 100), and without column 0 the new row reads 0 <= -1"""
    A, b, c = inst
    row = np.zeros(A.shape[1])
    row[0] = -1.0
    return np.ascontiguousarray(np.vstack([A, row])), np.append(100.0 * b, -1.0), c


def column_0_batch():
    """three (12, 11) instances of needing_column_0: in the first x_0 = 1 is basic in the new row itself,
    whose only other entry is the slack's -1 (no candidate: cold); in the others x_0 > 1 stands in another
    row, is forced out, and the dual loop finds the row 0 <= -1"""
    from batch_state_refs import warm_instances

    return [needing_column_0(inst) for inst in warm_instances(12, 10)[3:6]]


def mixed_batch():
    """24 (12, 10) instances in [-100, 100]: phase-1, UNBOUNDED and FEASIBLE in-states side by side"""
    return mixed_instances(12, 10)


def many_drops():
    """1,200 problems of (5, 5), row 4 - k % 5 ... each its own row: more than the resident workgroups"""
    return _once("drop-many", lambda: [oracle.generate(5, 5, 31 * s + 7, 1, 100) for s in range(1200)])


def in_class(kind, n_in, m_in, q):
    """(class of the in-state's shape, class of the reduced one)"""
    n, m = (n_in, m_in - q) if kind == ROWS else (n_in - q, m_in)
    return sx.batch_class(n_in, m_in), sx.batch_class(n, m)
