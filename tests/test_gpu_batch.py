"""Batched solve (simplex_solve_batch, sx_batch.hip) on the GPU: every problem of a call, whether
it ran inside a resident workgroup (LDS or workspace class) or on the engine, must give exactly
what twoPhaseMethodEx gives -- checked against the CPU oracle computed at test time: status, both
pivot counts and the basis match, and a FEASIBLE problem's objective and solution match as bit
patterns (the comparison of tests/test_gpu_degenerate_faults.py::solve_both).
"""
import json
import os

import numpy as np
import pytest

import oracle
import simplexoncuda_amd as sx
from conftest import GOLDEN, two_phase_ref

pytestmark = pytest.mark.gpu

RAGGED = [(1, 1), (2, 3), (5, 4), (20, 10), (16, 32), (33, 31), (64, 64), (65, 63)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_as_ref(got, ref):
    assert got.status == ref["status"]
    assert tuple(got.pivots) == ref["pivots"]
    assert np.array_equal(got.base, ref["base"])
    if got.status == sx.FEASIBLE:
        assert np.array_equal(bits(got.optimal_value), bits(ref["opt"]))
        assert np.array_equal(bits(got.solution), bits(ref["x"]))


def solve_batch(insts, max_pivots=-1):
    probs = [sx.Problem.from_arrays(*abc) for abc in insts]
    try:
        return sx.solve_batch(probs, max_pivots)
    finally:
        for p in probs:
            p.close()


def check_batch(insts):
    """one solve_batch call over insts [(A, b, c)], every result against the oracle; returns
    (results, oracle results)"""
    got = solve_batch(insts)
    refs = [two_phase_ref(*abc) for abc in insts]
    assert len(got) == len(insts)
    for g, r in zip(got, refs):
        same_as_ref(g, r)
    return got, refs


def predicted_split(insts):
    cls = [sx.batch_class(A.shape[1], A.shape[0]) for A, _, _ in insts]
    return cls.count(2), cls.count(1), cls.count(0)


def ragged_batch():
    return [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for n, m in RAGGED for s in (1, 2)]


def test_smallest_and_ragged_shapes(gpu):
    insts = ragged_batch()
    check_batch(insts)
    assert sx.batch_counts() == (len(insts), 0, 0, 0)


def test_mixed_outcomes(gpu):
    insts = [oracle.generate(n, m, seed * 7919 + n * 100 + m, -100, 100)
             for n, m in [(12, 9), (10, 20), (30, 30)] for seed in range(1, 9)]
    assert len({two_phase_ref(*abc)["status"] for abc in insts}) >= 3
    with open(os.path.join(GOLDEN, "degenerate_cases.json")) as f:
        small = json.load(f)["small"]
    assert len(small) == 4
    insts += [tuple(np.array(s[k], dtype=np.float64) for k in ("A", "b", "c")) for s in small]
    insts += [oracle.read_problem_text(os.path.join(GOLDEN, "examples", name))
              for name in ("smallProblem.txt", "infeasibleProblem.txt", "unboundedProblem.txt")]
    got, _ = check_batch(insts)
    assert [g.status for g in got[24:28]] == [sx.DEGENERATE] * 4
    assert [g.status for g in got[28:]] == [sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED]


def test_tile_and_block_boundaries(gpu):
    """the entering argmin at 512 / 513 values in phase 1 ((500, 6), (501, 6)) and around one tile
    in phase 2 ((505, 6), (506, 6), and (507, 6): 513 values); the ratio argmin and the objective
    GEMV at 512 / 513 rows ((4, 512), (4, 513)) -- each in the class batch_class assigns it"""
    shapes = [(500, 6), (501, 6), (505, 6), (506, 6), (507, 6), (4, 512), (4, 513)]
    insts = [oracle.generate(n, m, n * 100 + m, 1, 100) for n, m in shapes]
    check_batch(insts)
    split = predicted_split(insts)
    assert sx.batch_counts() == split + (0,)
    assert split[2] == 0  # all of them resident: these paths are the kernel's, not the engine's


def test_class_boundary(gpu):
    m = 64
    n = 1
    while sx.batch_class(n + 1, m) == 2:
        n += 1
    assert sx.batch_class(n, m) == 2 and sx.batch_class(n + 1, m) == 1
    insts = [oracle.generate(k, m, k * 100 + m, 1, 100) for k in (n, n + 1)]
    check_batch(insts)
    assert sx.batch_counts() == (1, 1, 0, 0)


def test_more_problems_than_resident_workgroups(gpu):
    """2,500 problems through the few hundred workgroups the device holds at once: the work counter
    hands out every index once and a workgroup's state is rebuilt for each problem it takes"""
    insts = [oracle.generate(5, 4, 50000 + s, 1, 100) for s in range(2500)]
    check_batch(insts)
    assert sx.batch_counts()[0] == 2500


def test_pivot_cap(gpu):
    insts = [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for n, m in [(20, 10), (64, 64)] for s in (1, 2)]
    got = solve_batch(insts, max_pivots=5)
    for g, abc in zip(got, insts):
        ref = oracle.two_phase(*abc, max_pivots=5)
        assert ref["status"] == sx.PIVOT_CAP
        same_as_ref(g, ref)
    assert sx.batch_counts() == (len(insts), 0, 0, 0)


def test_eviction(gpu):
    """a resident budget of 3 pivots per phase: every problem that needs a fourth pivot in either
    phase is marked by the kernel and re-solved on the engine; results do not change"""
    insts = ragged_batch()
    sx.set_batch_budget(3)
    try:
        _, refs = check_batch(insts)
        counts = sx.batch_counts()
    finally:
        sx.set_batch_budget(0)
    over = sum(1 for r in refs if max(r["pivots"]) > 3)
    assert 0 < over < len(insts)
    assert counts == (len(insts), 0, 0, over)


def test_no_leakage_into_single_problem_path(gpu):
    A, b, c = oracle.generate(20, 10, 2010, 1, 100)
    p = sx.Problem.from_arrays(A, b, c)
    try:
        before = sx.twoPhaseMethodEx(p)
        check_batch(ragged_batch())
        after = sx.twoPhaseMethodEx(p)
    finally:
        p.close()
    same_as_ref(before, two_phase_ref(A, b, c))
    assert before.status == after.status and tuple(before.pivots) == tuple(after.pivots)
    assert np.array_equal(before.base, after.base)
    assert np.array_equal(bits(before.optimal_value), bits(after.optimal_value))
    assert np.array_equal(bits(before.solution), bits(after.solution))


def test_engine_fallback(gpu):
    """one problem above the workspace cap between two small ones.  "Smallest" is taken as the
    class-0 shape with the fewest coefficients: one variable and the fewest constraints (the
    working set grows with m (n + m)); the oracle solves it in milliseconds"""
    m = 1
    while sx.batch_class(1, m) != 0:
        m += 1
    assert sx.batch_class(1, m - 1) == 1
    insts = [oracle.generate(20, 10, 2010, 1, 100), oracle.generate(1, m, 100 + m, 1, 100),
             oracle.generate(5, 4, 504, 1, 100)]
    check_batch(insts)
    assert sx.batch_counts() == (2, 0, 1, 0)
