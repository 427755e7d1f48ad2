"""A kept batch state grown by new structural columns (simplex_solve_batch_device_cols) restated from
batch_rhs_refs (_sum_partials, _enter_dual), batch_state_refs (_run, ref_state, _negative) and the
oracle's gemv_partials and argmin, and nothing else, for test_batch_cols_host.py (the oracle alone) and
test_gpu_batch_cols.py (bit for bit against the GPU).

A kept tableau is M [D b | D A | D], so its slack block is S = M D and the stored form of a new column
a is S a; its reduced cost is y a - c_new with y the slack entries of d.  Both sums are
batch_rhs_refs.new_rhs' sums with a in the place of b'.

A reference state is batch_state_refs' dict (phase 3 as in batch_rhs_refs), in the grown shape.  A
result that went through the dual loop has batch_rhs_refs' "dual"; "cold" says whether the problem was
solved from scratch.
"""
import numpy as np

import oracle
import simplexoncuda_amd as sx
from batch_rhs_refs import _enter_dual, _sum_partials
from batch_state_refs import _negative, _once, _run, ref_state, save_instances


def new_cols(state, A, c):
    """(the stored columns [m, p], their reduced costs [p]) of the columns n0 .. n of A [m, n] and
    c [n] on a phase-2 or phase-3 state of shape (n0, m): S a and y a - c_new, each sum gemv_partials'
    (ascending by fma from +0.0 in 512-element blocks), the blocks added left to right"""
    T0, d0 = state["T"], state["d"]
    m, Ns0 = T0.shape
    n0 = Ns0 - 1 - m
    n = A.shape[1]
    St = np.ascontiguousarray(T0[:, 1 + n0:].T)  # rows k, columns i: p[i] = fma(S[i][k], a[k], p[i])
    y = np.ascontiguousarray(d0[1 + n0:Ns0].reshape(m, 1))
    cols, red = np.zeros((m, n - n0)), np.zeros(n - n0)
    for t in range(n - n0):
        a = np.ascontiguousarray(A[:, n0 + t], dtype=np.float64)
        cols[:, t] = _sum_partials(oracle.gemv_partials(St, a, m))
        red[t] = _sum_partials(oracle.gemv_partials(y, a, 1))[0] - c[n0 + t]
    return cols, red


def grown_tableau(state, A, c):
    """(T [m, 1 + n + m], d [1 + n + 2m], base) of a phase-2 or phase-3 state with the new columns in
    place: the structural block grows in the middle, the slack columns and the basic slacks' indices
    move up by p, d is +0.0 from 1 + n + m on"""
    T0, d0, base0 = state["T"], state["d"], state["base"]
    m, Ns0 = T0.shape
    n0 = Ns0 - 1 - m
    n = A.shape[1]
    p, Ns = n - n0, 1 + n + m
    T, d = np.zeros((m, Ns)), np.zeros(Ns + m)
    T[:, :1 + n0] = T0[:, :1 + n0]
    T[:, 1 + n:] = T0[:, 1 + n0:]
    d[:1 + n0] = d0[:1 + n0]
    d[1 + n:Ns] = d0[1 + n0:Ns0]
    T[:, 1 + n0:1 + n], d[1 + n0:1 + n] = new_cols(state, A, c)
    base = np.where(base0 >= n0, base0 + p, base0).astype(np.int32)
    return T, d, base


def ref_cols(state, A, b, c, max_pivots=-1):
    """the grown state and results of `state` (shape (n0, m), left as it is) with the columns n0 .. n of
    A [m, n] and c [n] appended"""
    m, Ns0 = state["T"].shape
    n0 = Ns0 - 1 - m
    n = A.shape[1]
    assert A.shape[0] == m and n > n0 >= 1
    res = None
    if state["phase"] != 1:
        T, d, base = grown_tableau(state, A, c)
        first = (state["pivots"][0], 0)
        if state["phase"] == 2:  # the old basis is primal feasible: always warm
            res = _run(T, d, base, 2, first, c, max_pivots, False)
        elif not _negative(oracle.argmin(d[1:1 + n + m])[1]):  # phase 3, still dual feasible
            res = _enter_dual(T, d, base, first, c, max_pivots, oracle.argmin)
    cold = res is None
    if cold:
        res = dict(ref_state(A, b, c, max_pivots))  # (its arrays are shared: do not write them)
    res["cold"] = cold
    return res


# ---- the instances both test files use ----
def lds_edge(m=64):
    """n0 with (n0, m) in the LDS class and (n0 + 1, m) in the workspace class"""
    n0 = 1
    while sx.batch_class(n0 + 1, m) == 2:
        n0 += 1
    assert sx.batch_class(n0, m) == 2 and sx.batch_class(n0 + 1, m) == 1
    return n0


def cols_shapes():
    """(n0, p, m): the base cases ((5, 3, 4) is p = 3), a grown class edge at 64 columns, LDS to
    workspace -- at m = 64 that edge is n0 = 240, so (240, 1, 64) is this case and (241, 1, 64) is
    workspace to workspace --, the leaving ratio over two row tiles, the new column the last candidate
    of the first entering tile and the first of the second, entering selection over two tiles"""
    edge = lds_edge(64)
    shapes = [(1, 1, 1), (5, 1, 4), (5, 3, 4), (20, 1, 10), (33, 1, 31), (63, 1, 64), (edge, 1, 64), (240, 1, 64),
              (241, 1, 64), (4, 1, 513), (511, 1, 4), (512, 1, 4), (599, 1, 4)]
    return [s for k, s in enumerate(shapes) if s not in shapes[:k]]


THETAS = [0.01, 100.0]
KINDS = [("scaled", 0.01), ("scaled", 100.0), ("unbounded", 1.0)]
CAP_SHAPE = (63, 1, 64)  # the second and third instance make more than 8 warm pivots at theta = 100
CAP_KEEP = [1, 2]
COLS_CAPS = [1, 2, 8]
RESCUE_SHAPES = [(5, 4), (20, 10), (33, 31), (63, 64)]


def grown_instances(n0, p, m):
    """three generated instances in [1, 100] of the grown shape (batch_state_refs' draws)"""
    return save_instances(n0 + p, m)


def kept_part(inst, n0):
    """the problem a state is kept of: the first n0 columns (views: on the GPU a slice exercises strides)"""
    A, b, c = inst
    return np.ascontiguousarray(A[:, :n0]), b, np.ascontiguousarray(c[:n0])


def with_new(inst, n0, kind, theta):
    """the grown instance as a call gets it: the new columns' costs scaled by theta, or (unbounded) the
    new columns of A negated -- a non-positive column with a positive cost -- and the costs as drawn"""
    A, b, c = inst
    A, c = A.copy(), c.copy()
    if kind == "unbounded":
        A[:, n0:] = -A[:, n0:]
    else:
        c[n0:] = theta * c[n0:]
    return A, b, c


def want_batch(n0, p, m, kind, theta, max_pivots=-1):
    """the kept parts of a shape's three instances, the grown instances, the kept states and what adding
    the columns must give, computed once: (kept, grown, [ref_state], [ref_cols]); do not write them"""
    def make():
        insts = grown_instances(n0, p, m)
        kept = [kept_part(inst, n0) for inst in insts]
        grown = [with_new(inst, n0, kind, theta) for inst in insts]
        refs = [ref_state(*k) for k in kept]
        return kept, grown, refs, [ref_cols(r, *g, max_pivots) for r, g in zip(refs, grown)]
    return _once(("cols-want", n0, p, m, kind, theta, max_pivots), make)


def elastic(inst, cost):
    """the instance with one elastic column: -1 in row 0, zeros elsewhere, the given cost"""
    A, b, c = inst
    col = np.zeros((A.shape[0], 1))
    col[0, 0] = -1.0
    return np.ascontiguousarray(np.hstack([A, col])), b, np.append(c, cost)


def generated_column(m, seed, theta):
    """one generated column in [1, 100] with its cost scaled by theta: (a [m, 1], cost)"""
    A, _, c = _once(("col", m, seed), lambda: oracle.generate(1, m, seed, 1, 100))
    return A.copy(), theta * c[0]


def append_column(inst, seed, theta):
    """the instance with one generated column appended"""
    A, b, c = inst
    a, cost = generated_column(A.shape[0], seed, theta)
    return np.ascontiguousarray(np.hstack([A, a])), b, np.append(c, cost)


def many_grown():
    """1,200 problems of (6, 4), kept as (5, 4): more than the resident workgroups"""
    return _once("cols-many", lambda: [with_new(oracle.generate(6, 4, 31 * s + 7, 1, 100), 5, "scaled", 100.0)
                                       for s in range(1200)])
