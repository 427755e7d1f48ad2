"""The structured family (structured_lps.py: b = 0, zero and non-positive costs, zero rows and columns,
duplicate constraints, b just below zero and -0.0, subnormal and 2^900-scaled rows, subnormal costs)
through every entry (needs an MI355X).  Each instance is compared with the oracle's result under the
same pivot cap, with the final objective row, bit for bit and without a tolerance.  Every call runs
with max_pivots = 4 (n + m) (the ragged call: the envelope's), which no instance reaches on the
oracle (test_structured_lps.py): a kernel that cycled on a degenerate LP would end, and fail."""
import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
import structured_lps as sl
import test_gpu_batch_ragged as rag
import test_gpu_solve_device as tsd
from batch_refs import bits, ref_with_row, same_as_refs, tensors

pytestmark = pytest.mark.gpu


def shape_refs(n, m, cap):
    insts = [inst for _, _, inst in sl.of_shape(n, m)]
    return insts, [ref_with_row(*inst, max_pivots=cap) for inst in insts]


@pytest.mark.parametrize("n,m", sl.SHAPES)
def test_one_shape_entry(gpu, n, m):
    insts, refs = shape_refs(n, m, sl.cap(n, m))
    A, b, c = tensors(insts)
    keep = [t.clone() for t in (A, b, c)]
    out = sx.solve_batch_tensors(A, b, c, max_pivots=sl.cap(n, m), objective_row=True)
    same_as_refs(out, refs, n, m)
    assert out.evicted == 0
    assert all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip((A, b, c), keep))  # -0.0 stays


def test_ragged_entry_all_in_one_envelope(gpu):
    n, m = 33, 33
    assert all(nk <= n and mk <= m for nk, mk in sl.SHAPES)
    insts = [inst for *_, inst in sl.family()]
    out, refs = rag.check(insts, n, m, max_pivots=sl.cap(n, m))
    assert len(refs) == 88 and out.evicted == 0
    assert {r["status"] for r in refs} == {sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED, sx.DEGENERATE}


@pytest.mark.parametrize("n,m", sl.SHAPES)
def test_host_batch_entry(gpu, n, m):
    insts, refs = shape_refs(n, m, sl.cap(n, m))
    probs = [sx.Problem.from_arrays(*inst) for inst in insts]
    try:
        got = sx.solve_batch(probs, sl.cap(n, m))
    finally:
        for p in probs:
            p.close()
    assert sx.batch_counts() == (len(insts), 0, 0, 0)
    for k, (g, ref) in enumerate(zip(got, refs)):
        assert g.status == ref["status"] and tuple(g.pivots) == ref["pivots"], k
        assert np.array_equal(g.base, ref["base"]), k
        if ref["status"] == sx.FEASIBLE:
            assert bits(g.optimal_value) == bits(ref["opt"]) and np.array_equal(bits(g.solution), bits(ref["x"])), k


@pytest.mark.parametrize("blocked", [-1, 0])
@pytest.mark.parametrize("n,m", sl.SHAPES)
def test_solve_tensors(gpu, n, m, blocked):
    insts, refs = shape_refs(n, m, sl.cap(n, m))
    try:
        sx.set_blocked(blocked)
        for k, (inst, ref) in enumerate(zip(insts, refs)):
            out = sx.solve_tensors(*(tsd.dev(a) for a in inst), max_pivots=sl.cap(n, m), objective_row=True)
            try:
                tsd.compare(out, ref, n, m, out.solution.device)
            except AssertionError as e:
                raise AssertionError(f"instance {k}: {sl.of_shape(n, m)[k][:2]}") from e
    finally:
        sx.set_blocked(-1)


@pytest.mark.parametrize("n,m", sl.SHAPES)
def test_two_phase_method_ex(gpu, n, m):
    insts, refs = shape_refs(n, m, sl.cap(n, m))
    for k, (inst, ref) in enumerate(zip(insts, refs)):
        p = sx.Problem.from_arrays(*inst)
        try:
            g = sx.twoPhaseMethodEx(p, sl.cap(n, m))
            row = sx.last_objective_row()
        finally:
            p.close()
        who = sl.of_shape(n, m)[k][:2]
        assert g.status == ref["status"] and tuple(g.pivots) == ref["pivots"], who
        assert np.array_equal(g.base, ref["base"]), who
        assert np.array_equal(bits(row), bits(ref["row"])), who
        if ref["status"] == sx.FEASIBLE:
            assert bits(g.optimal_value) == bits(ref["opt"]) and np.array_equal(bits(g.solution), bits(ref["x"])), who


@pytest.mark.parametrize("blocked", [-1, 0])
def test_build_keeps_tiny_negative_and_minus_zero(gpu, blocked):
    """b_tiny_neg through the engine's device build: a row with b = -1e-12 is not negated (the build
    negates below -eps, while slack compaction is decided by b < 0.0), and b = -0.0 stays -0.0"""
    try:
        sx.set_blocked(blocked)
        for n, m in sl.SHAPES:
            for s in sl.SEEDS:
                A, b, _ = sl.instance("b_tiny_neg", n, m, s)
                ref = oracle.build_phase1(A, b)
                T, d, base = sx.dev_build_phase1_tensors(tsd.dev(A), tsd.dev(b))
                assert tsd.same(T, ref[0]) and tsd.same(d, ref[1]) and np.array_equal(base, ref[2])
                assert np.array_equal(bits(T[:, 0]), bits(b)) and tsd.same(T[:, 1:1 + n], A)  # no row negated
                assert (T[1::3, 0] == 0).all() and np.signbit(T[1::3, 0]).all()
    finally:
        sx.set_blocked(-1)
