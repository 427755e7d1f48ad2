"""A kept batch state grown by new constraint rows (simplex_solve_batch_device_rows) restated from
batch_state_refs / batch_rhs_refs (_dual and _run through _enter_dual, dual_feasible's selection,
ref_state for the cold start) and the oracle's pieces, and nothing else, for test_batch_rows_host.py
(the oracle alone) and test_gpu_batch_rows.py (bit for bit against the GPU).

The fma chain of a new row is the oracle's own fma: orc_apply_update's objective-row step with the
pivot 1.0 is d[j] = fma(-d_e, prow[j], d[j]), so one call per old row, in ascending order, is the
chain acc_j = fma(-f_i, T[i][j], acc_j) (numpy has no fused multiply-add).

A reference state is batch_state_refs' dict (phase 3 as in batch_rhs_refs), in the grown shape.
"""
import numpy as np

import oracle
import simplexoncuda_amd as sx
from batch_rhs_refs import _enter_dual
from batch_state_refs import _negative, _once, ref_state, save_instances


def new_rows(state, A, b):
    """the stored rows m0 .. m of the grown tableau, [q, 1 + n + m]: the raw row R = b | A | unit, minus
    f_i times old row i (padded with +0.0) for i = 0 .. m0 - 1 in that order, each step one fma"""
    T0, base = state["T"], state["base"]
    m0, Ns0 = T0.shape
    m, n = A.shape
    Ns = 1 + n + m
    old = np.zeros((m0, Ns))
    old[:, :Ns0] = T0
    rows = np.zeros((m - m0, Ns))
    one = np.zeros(1)
    for t in range(m - m0):
        acc = rows[t]
        acc[0] = b[m0 + t]
        acc[1:1 + n] = A[m0 + t]
        acc[1 + n + m0 + t] = 1.0
        for i in range(m0):
            f = A[m0 + t, base[i]] if base[i] < n else 0.0
            keep = old[i:i + 1].copy()  # (the call rewrites its pivot row as prow / 1.0)
            oracle.apply_update(keep, acc, old[i], one, 0, 1.0, f)
    return rows


def grown_dual_feasible(state, q):
    """the entering eps-argmin over the grown d[1 .. Ns) -- the state's entries, then q of +0.0 -- does
    not compare below zero (batch_rhs_refs.dual_feasible's test at the grown width)"""
    Ns0 = state["T"].shape[1]
    return not _negative(oracle.argmin(np.concatenate([state["d"][1:Ns0], np.zeros(q)]))[1])


def ref_rows(state, A, b, c, max_pivots=-1, argmin=oracle.argmin, enter_argmin=None, leave_argmin=None):
    """the grown state and results of `state` (shape (n, m0), left as it is) with the rows m0 .. m of
    A [m, n] and b [m] appended; argmin: the selection of the dual loop, enter_argmin / leave_argmin: one
    for its entering ratio / its leaving row alone (batch_rhs_refs.ref_rhs)"""
    m0, Ns0 = state["T"].shape
    m, n = A.shape
    q = m - m0
    assert q >= 1 and Ns0 == 1 + n + m0
    if state["phase"] == 1 or not grown_dual_feasible(state, q):
        return ref_state(A, b, c, max_pivots)  # the cold start (shared: do not write it)
    Ns = 1 + n + m
    T = np.zeros((m, Ns))
    T[:m0, :Ns0] = state["T"]
    T[m0:] = new_rows(state, A, b)
    d = np.zeros(Ns + m)
    d[:Ns0] = state["d"][:Ns0]
    base = np.concatenate([state["base"], n + m0 + np.arange(q)]).astype(np.int32)
    return _enter_dual(T, d, base, (state["pivots"][0], 0), c, max_pivots, argmin, enter_argmin, leave_argmin)


# ---- the instances both test files use ----
def lds_edge(n=241):
    """m0 with (n, m0) in the LDS class and (n, m0 + 1) in the workspace class"""
    m0 = 1
    while sx.batch_class(n, m0 + 1) == 2:
        m0 += 1
    assert sx.batch_class(n, m0) == 2 and sx.batch_class(n, m0 + 1) == 1
    return m0


def rows_shapes():
    """(n, m0, q): the base cases ((5, 4, 3) is q = 3), a grown class edge at 64 rows, LDS to workspace,
    workspace to workspace, the new row as the first of a second row tile of the leaving argmin, and
    the entering ratio over two tiles"""
    return [(1, 1, 1), (5, 4, 1), (5, 4, 3), (20, 10, 1), (33, 31, 1), (64, 63, 1), (241, lds_edge(241), 1), (241, 64, 1),
            (4, 512, 1), (600, 4, 1)]


THETAS = [0.5, 1.5]
KINDS = ["cut", "down", "up"]
CAP_SHAPE = (241, lds_edge(241), 1)  # every theta = 0.5 cut makes more than 8 dual pivots there
ROWS_CAPS = [1, 2, 8]


def rows_instances(n, m0):
    """three generated instances in [1, 100] (batch_state_refs' draws)"""
    return save_instances(n, m0)


def optimum(inst):
    """x* of a [1, 100] instance's oracle optimum"""
    st = ref_state(*inst)
    assert st["status"] == oracle.FEASIBLE
    return st["x"]


def positive_row(n, seed):
    """one generated row in [1, 100]"""
    return _once(("row", n, seed), lambda: oracle.generate(n, 1, seed, 1, 100)[0][0].copy())


def make_row(inst, kind, theta, seed=0):
    """(a, beta) of one new row a x <= beta for the instance, from its optimum x*:
      cut   a generated positive row, beta = theta a x*           (cuts x* off when theta < 1)
      down  e_j on the structural variable with the largest x*_j, beta = theta x*_j     (theta < 1)
      up    -e_j on the same variable, beta = -theta x*_j         (cuts x* off when theta > 1)
      never a generated positive row, beta = -1: no x >= 0 satisfies it"""
    A, _, _ = inst
    n = A.shape[1]
    x = optimum(inst)
    if kind in ("cut", "never"):
        a = positive_row(n, 7000 + 13 * seed + n)
        return a, (-1.0 if kind == "never" else theta * float(a @ x))
    j = int(np.argmax(x))
    a = np.zeros(n)
    a[j] = 1.0 if kind == "down" else -1.0
    return a, a[j] * theta * x[j]


def cuts_off(kind, theta):
    """the row excludes x*: the warm start has to pivot in the dual loop"""
    return kind == "never" or (theta > 1.0 if kind == "up" else theta < 1.0)


def grow(inst, kinds, theta):
    """the instance with one new row per entry of `kinds` appended: (A [m0 + q, n], b [m0 + q], c)"""
    A, b, c = inst
    rows = [make_row(inst, kind, theta, seed=t) for t, kind in enumerate(kinds)]
    return (np.ascontiguousarray(np.vstack([A] + [a for a, _ in rows])), np.concatenate([b, [beta for _, beta in rows]]),
            c)


def kinds_for(q, kind="cut"):
    """q rows of one kind: cuts are drawn with one seed each, a branch row is repeated (equal rows tie
    in the dual loop's leaving selection)"""
    return [kind] * q


def grown_batch(n, m0, q, kind, theta):
    """the three instances of a shape, grown: ([(A0, b0, c)], [(A, b, c)])"""
    insts = rows_instances(n, m0)
    return insts, [grow(inst, kinds_for(q, kind), theta) for inst in insts]


def want_batch(n, m0, q, kind, theta, max_pivots=-1):
    """grown_batch with the kept states of the instances and what adding the rows must give, computed
    once: (insts, grown, [ref_state], [ref_rows]); do not write them"""
    def make():
        insts, grown = grown_batch(n, m0, q, kind, theta)
        refs = [ref_state(*inst) for inst in insts]
        return insts, grown, refs, [ref_rows(r, *g, max_pivots) for r, g in zip(refs, grown)]
    return _once(("want", n, m0, q, kind, theta, max_pivots), make)
