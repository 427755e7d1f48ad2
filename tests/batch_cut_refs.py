"""Gomory mixed-integer cuts from a kept batch state (simplex_solve_batch_device_cut) restated from
batch_rows_refs (ref_rows: the rows entry on the explicit grown problem), the oracle's eps-argmin tree
and the oracle's fma, and nothing else, for test_batch_cut_host.py (the oracle alone) and
test_gpu_batch_cut.py (bit for bit against the GPU).

The fma chain of a cut's row in the caller's variables is the oracle's own fma, as in
batch_rows_refs.new_rows: orc_apply_update's objective-row step with the pivot 1.0 is
d[j] = fma(-d_e, prow[j], d[j]), so with d_e = -g one call per old row i, in ascending order, is the
chain acc_j = fma(g_{n+i}, A[i][j], acc_j), the right-hand side riding along as column n.

A reference state is batch_state_refs' dict (phase 3 as in batch_rhs_refs).
"""
import math

import numpy as np

import oracle
from batch_rhs_refs import DBL_MAX
from batch_rows_refs import grown_dual_feasible, ref_rows
from batch_state_refs import EPS, _once, mixed_instances, ref_state, save_instances

AWAY = 0.05
SCALES = [1, 37]


def _compare0(x):
    """compare(x, 0) (macro.h)"""
    return 0 if abs(x) < EPS else (-1 if x < 0 else 1)


def frac(t):
    return t - math.floor(t)


def usable(state, q):
    """a kept optimum: phase 2 and the rows entry's warm test at the grown width"""
    return state["phase"] == 2 and grown_dual_feasible(state, q)


def row_keys(state, integer, away, taken=()):
    """the key of every row of the state: -min(f0, 1 - f0) for an eligible row, DBL_MAX otherwise"""
    T, base = state["T"], state["base"]
    m0 = T.shape[0]
    n = T.shape[1] - 1 - m0
    keys = np.full(m0, DBL_MAX)
    for i in range(m0):
        v = int(base[i])
        if v >= n or not integer[v] or i in taken:
            continue
        f0 = frac(T[i, 0])
        if f0 >= away and 1.0 - f0 >= away:
            keys[i] = -min(f0, 1.0 - f0)
    return keys


def gmi(state, integer, r):
    """(g over the stored columns [0, n + m0), f0) of source row r"""
    T, base = state["T"], state["base"]
    m0 = T.shape[0]
    n = T.shape[1] - 1 - m0
    f0 = frac(T[r, 0])
    rho = f0 / (1.0 - f0)
    basic = set(int(v) for v in base)
    g = np.zeros(n + m0)
    for jj in range(n + m0):
        al = T[r, 1 + jj]
        if jj in basic or _compare0(al) == 0:
            continue
        if jj < n and integer[jj]:
            fj = frac(al)
            g[jj] = fj if fj <= f0 else rho * (1.0 - fj)
        else:
            g[jj] = al if al > 0 else rho * (-al)
    return g, f0


def in_callers_variables(g, f0, A0, b0):
    """(cut_A [n], cut_b) of sum g v >= f0 with the slacks s_i = b_i - A_i x substituted: from -g_j
    (-f0), acc = fma(g_{n+i}, A[i][j] (b[i]), acc) for i = 0 .. m0 - 1 in that order"""
    m0, n = A0.shape
    acc = np.concatenate([-g[:n], [-f0]])
    one = np.zeros(1)
    for i in range(m0):
        prow = np.concatenate([A0[i], [b0[i]]])
        keep = prow.reshape(1, n + 1).copy()  # (the call rewrites its pivot row as prow / 1.0)
        oracle.apply_update(keep, acc, prow, one, 0, 1.0, -g[n + i])
    return acc[:n].copy(), float(acc[n])


def ref_cut(state, A0, b0, c, integer, q, away=AWAY, rows=None, max_pivots=-1, argmin=oracle.argmin):
    """(cut_A [q, n], cut_b [q], cut_row int32 [q], ref_rows of the grown problem) of `state` (shape
    (n, m0), left as it is), solved with A0 [m0, n], b0 [m0]; integer: a mask [n]; rows: the caller's
    source rows [q] or None; argmin: the selection of the source row, the oracle's eps-argmin tree unless
    a test swaps it"""
    m0, n = A0.shape
    assert state["T"].shape == (m0, 1 + n + m0) and q >= 1
    integer = np.asarray(integer).astype(bool)
    cut_A, cut_b = np.zeros((q, n)), np.zeros(q)
    cut_row = np.full(q, -1, dtype=np.int32)
    if usable(state, q):
        taken = set()
        for t in range(q):
            keys = row_keys(state, integer, away, taken)
            if rows is None:
                r, v = argmin(keys)
                if v == DBL_MAX or r < 0:
                    continue
            else:
                r = int(rows[t])
                if not 0 <= r < m0 or keys[r] == DBL_MAX:
                    continue
            g, f0 = gmi(state, integer, r)
            cut_A[t], cut_b[t] = in_callers_variables(g, f0, A0, b0)
            cut_row[t] = r
            taken.add(r)
    A = np.ascontiguousarray(np.vstack([A0, cut_A]))
    b = np.concatenate([b0, cut_b])
    return cut_A, cut_b, cut_row, ref_rows(state, A, b, c, max_pivots)


# ---- the instances both test files use ----
def masks(n):
    """all-integer, every second variable, none"""
    return {"all": np.ones(n, dtype=bool), "second": np.arange(n) % 2 == 0, "none": np.zeros(n, dtype=bool)}


def cut_instances(n, m0, scale):
    """batch_state_refs.save_instances with b times `scale` (scale 1: x* < 1 everywhere)"""
    return _once(("cut", n, m0, scale), lambda: [(A, b * float(scale), c) for A, b, c in save_instances(n, m0)])


def want_cut(n, m0, q, scale, mask="all", max_pivots=-1):
    """the three instances of a shape, their kept states and what cutting them must give, computed
    once: (insts, [ref_state], [ref_cut]); do not write them"""
    def make():
        insts = cut_instances(n, m0, scale)
        refs = [ref_state(*inst) for inst in insts]
        return insts, refs, [ref_cut(r, inst[0], inst[1], inst[2], masks(n)[mask], q, AWAY, None, max_pivots)
                             for r, inst in zip(refs, insts)]
    return _once(("want-cut", n, m0, q, scale, mask, max_pivots), make)


def mixed_cut_instances():
    """batch_state_refs.mixed_instances: phase-1, UNBOUNDED and FEASIBLE states side by side"""
    return mixed_instances()


def grown_arrays(inst, cut):
    """the explicit grown problem of an instance and its ref_cut"""
    A0, b0, c = inst
    return np.ascontiguousarray(np.vstack([A0, cut[0]])), np.concatenate([b0, cut[1]]), c
