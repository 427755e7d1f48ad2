"""Branching a kept batch state (simplex_solve_batch_device_branch) restated through
batch_rows_refs.ref_rows on the explicit child, and nothing else, for test_batch_branch_host.py (the
oracle alone) and test_gpu_batch_branch.py (bit for bit against the GPU).

A child is a root instance (A [mA, n], b [mA], c) followed by q bound rows, given as three lists of
length q: coef[t] * x[var[t]] <= rhs[t].  The entry is defined as the rows entry with one new row on the
explicit grown problem -- the bound rows dense, coef at column var and +0.0 elsewhere -- so the
reference builds that problem (explicit) and calls ref_rows; a reference state is batch_state_refs' dict.
"""
import numpy as np

import oracle
from batch_rows_refs import CAP_SHAPE, lds_edge, make_row, ref_rows, rows_instances, rows_shapes
from batch_state_refs import _once, many_instances, mixed_instances, ref_state


def explicit(root_inst, var, coef, rhs):
    """the child as a dense problem: (A [mA + q, n], b [mA + q], c)"""
    A, b, c = root_inst
    n = A.shape[1]
    rows = np.zeros((len(var), n))
    for t, (j, v) in enumerate(zip(var, coef)):
        rows[t, int(j)] = v
    return (np.ascontiguousarray(np.vstack([A, rows])), np.concatenate([b, np.asarray(rhs, dtype=np.float64)]), c)


def ref_branch(state, root_inst, var, coef, rhs, max_pivots=-1, argmin=oracle.argmin, enter_argmin=None,
               leave_argmin=None):
    """the state and results of the child of `state` (left as it is): the bound rows that `state` does
    not hold yet -- for the entry that is the last one alone -- appended one at a time by ref_rows, which
    takes the selections argmin, enter_argmin and leave_argmin"""
    mA = root_inst[0].shape[0]
    q = len(var)
    have = state["T"].shape[0] - mA
    assert 0 <= have < q and len(coef) == q and len(rhs) == q
    for t in range(have, q):
        A, b, c = explicit(root_inst, var[:t + 1], coef[:t + 1], rhs[:t + 1])
        state = ref_rows(state, A, b, c, max_pivots, argmin, enter_argmin, leave_argmin)
    return state


def is_cold(ref):
    """the reference took the cold start (ref_state's dict says nothing about a dual loop)"""
    return "dual" not in ref


# ---- the instances both test files use ----
THETAS = [0.5, 1.5]
PARENTS = [[0, 0, 1, 1, 2, 2], [2, 0, 2, 0, 0, 2]]  # two children each; repeated, permuted, parent 1 left out
EDGE_SHAPES = [(5, 4), (241, lds_edge(241))]          # also compared with add_rows_batch_tensors


def branch_shapes():
    """(n, m0) of batch_rows_refs.rows_shapes() with one new row"""
    return [(n, m0) for n, m0, q in rows_shapes() if q == 1]


def bound(inst, kind, theta):
    """(j, coef, rhs) of batch_rows_refs.make_row's branch row: `down` is x_j <= theta x*_j, `up` is
    -x_j <= -theta x*_j, on the variable with the largest x*_j"""
    a, beta = make_row(inst, kind, theta)
    j = int(np.flatnonzero(a)[0])
    return j, float(a[j]), float(beta)


def two_children(insts, parent, theta):
    """child k is `down` (k even) or `up` (k odd) through the optimum of instance parent[k]:
    (var [C, 1] int32, coef [C, 1], rhs [C, 1])"""
    rows = [bound(insts[p], "down" if k % 2 == 0 else "up", theta) for k, p in enumerate(parent)]
    return (np.array([[r[0]] for r in rows], dtype=np.int32), np.array([[r[1]] for r in rows]),
            np.array([[r[2]] for r in rows]))


def want_children(states, roots, parent, root, var, coef, rhs, max_pivots=-1):
    """[ref_branch] of every child: states[parent[k]] on roots[root[k]]"""
    return [ref_branch(states[p], roots[r], var[k], coef[k], rhs[k], max_pivots)
            for k, (p, r) in enumerate(zip(parent, root))]


def want_two_children(n, m0, parent, theta, max_pivots=-1):
    """the instances of a shape, their kept states, the two_children triples and what the branch must
    give, computed once: (insts, refs, (var, coef, rhs), [ref_branch]); do not write them"""
    def make():
        insts = rows_instances(n, m0)
        refs = [ref_state(*inst) for inst in insts]
        tri = two_children(insts, parent, theta)
        return insts, refs, tri, want_children(refs, insts, parent, parent, *tri, max_pivots)
    return _once(("branch", n, m0, tuple(parent), theta, max_pivots), make)


# cold and warm in one call, and depth: mixed_instances(12, 9)
LEVEL1 = (0, 1.0, 10.0)    # 1 x_0 <= 10
LEVEL2 = (1, -1.0, -1.0)   # -1 x_1 <= -1


def mixed_levels():
    """(insts, [ref_state], [level 1], [level 2]) of the 24 mixed instances: level 1 adds LEVEL1 to every
    root state, level 2 adds LEVEL2 to level 1's out-state (q = 2)"""
    def make():
        insts = mixed_instances(12, 9)
        refs = [ref_state(*inst) for inst in insts]
        one = [ref_branch(r, inst, *zip(LEVEL1)) for r, inst in zip(refs, insts)]
        two = [ref_branch(s, inst, *zip(LEVEL1, LEVEL2)) for s, inst in zip(one, insts)]
        return insts, refs, one, two
    return _once("branch-mixed", make)


def many_parents():
    """the first 1200 of many_instances() (all of them) and two children each: C = 2400"""
    insts = many_instances()[:1200]
    parent = [k // 2 for k in range(2 * len(insts))]
    return insts, parent


def scratch(root_inst, var, coef, rhs):
    """oracle.two_phase on the explicit child"""
    return oracle.two_phase(*explicit(root_inst, var, coef, rhs))
