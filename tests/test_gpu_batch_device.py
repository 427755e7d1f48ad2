"""Device-resident batched solve (simplex_solve_batch_device, sx_batch.hip k_batch_solve_dev)
through sx.solve_batch_tensors: tensors in, tensors out.  Every problem of every call is compared
with the CPU oracle computed at test time, bit for bit and without a tolerance (batch_refs.py
same_as_refs, shared with test_gpu_batch_ladders.py):

  always                       status, both pivot counts, the basis
  FEASIBLE                     objective and solution as uint64 bit patterns
  otherwise                    the solution is all +0.0 and the objective a NaN
  with objective_row=True      row_width == len(oracle row), the row's bits, +0.0 behind row_width
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_refs import bits, ref_with_row, same_as_refs, same_tensors, tensors
from conftest import GOLDEN, two_phase_ref

pytestmark = pytest.mark.gpu


def check(insts, max_pivots=-1):
    """one solve_batch_tensors call over contiguous tensors with the objective row; returns
    (BatchTensors, oracle results)"""
    A, b, c = tensors(insts)
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True)
    refs = [ref_with_row(*abc, max_pivots=max_pivots) for abc in insts]
    m, n = insts[0][0].shape
    same_as_refs(out, refs, n, m)
    return out, refs


@pytest.mark.parametrize("n,m", [(1, 1), (2, 3), (5, 4), (20, 10), (33, 31), (64, 64), (65, 63)])
def test_smallest_and_odd_shapes(gpu, n, m):
    insts = [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2, 3)]
    assert sx.batch_class(n, m) == 2
    out, refs = check(insts)
    assert out.evicted == 0
    assert out.duals.shape == (3, m) and out.reduced_costs.shape == (3, n)
    # without the row: the same results, and no row
    plain = sx.solve_batch_tensors(*tensors(insts))
    assert plain.objective_row is None and plain.row_width is None and plain.evicted == 0
    same_as_refs(plain, refs, n, m)


def test_strided_inputs_are_read_in_place(gpu):
    n, m, B = 20, 10, 5
    insts = [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in range(1, B + 1)]
    A, b, c = tensors(insts)
    want, _ = check(insts)

    # a transposed view of a [B, n, m] tensor: the column (variable) stride exceeds the row stride
    At = A.transpose(1, 2).contiguous()
    keep = At.clone()
    view = At.transpose(1, 2)
    assert view.shape == A.shape and view.stride() == (n * m, 1, m)
    same_tensors(sx.solve_batch_tensors(view, b, c, objective_row=True), want)
    assert torch.equal(At, keep)

    # every second problem of tensors twice as long: the batch stride is not the dense one
    A2, b2, c2 = (torch.full((2 * B,) + tuple(t.shape[1:]), 7.0, dtype=torch.float64, device="cuda") for t in (A, b, c))
    A2[::2], b2[::2], c2[::2] = A, b, c
    keep = [t.clone() for t in (A2, b2, c2)]
    assert A2[::2].stride() == (2 * n * m, n, 1) and b2[::2].stride() == (2 * m, 1)
    same_tensors(sx.solve_batch_tensors(A2[::2], b2[::2], c2[::2], objective_row=True), want)
    assert all(torch.equal(t, k) for t, k in zip((A2, b2, c2), keep))

    # a column slice of a wider tensor: the row stride is not n
    wide = torch.full((B, m, 30), -3.0, dtype=torch.float64, device="cuda")
    wide[:, :, 3:23] = A
    keep = wide.clone()
    view = wide[:, :, 3:23]
    assert view.stride() == (m * 30, 30, 1)
    same_tensors(sx.solve_batch_tensors(view, b, c, objective_row=True), want)
    assert torch.equal(wide, keep)
    assert all(torch.equal(t, torch.from_numpy(np.stack([inst[k] for inst in insts])).cuda())
               for k, t in enumerate((A, b, c)))


def mixed(n, m):
    return [oracle.generate(n, m, s * 7919 + n * 100 + m, -100, 100) for s in range(1, 25)]


@pytest.mark.parametrize("n,m", [(12, 9), (30, 30)])
def test_mixed_outcomes_in_one_call(gpu, n, m):
    """FEASIBLE, INFEASIBLE and UNBOUNDED problems side by side: phase-1 rows (the Farkas rows of
    the infeasible ones, width 1 + n + 2m) and phase-2 rows in one output tensor"""
    insts = mixed(n, m)
    out, refs = check(insts)
    assert {r["status"] for r in refs} == {sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED}
    assert {len(r["row"]) for r in refs} == {1 + n + m, 1 + n + 2 * m}
    assert out.evicted == 0


def test_degenerate_cases(gpu):
    with open(os.path.join(GOLDEN, "degenerate_cases.json")) as f:
        small = json.load(f)["small"]
    assert len(small) == 4
    for s in small:
        inst = tuple(np.array(s[k], dtype=np.float64) for k in ("A", "b", "c"))
        out, _ = check([inst])
        assert out.status.tolist() == [sx.DEGENERATE]


def test_more_problems_than_resident_workgroups(gpu):
    """1,200 problems through the 512 workgroups 256 compute units hold at once: the work counter
    wraps the grid at least twice and a workgroup's state is rebuilt for each problem it takes"""
    insts = [oracle.generate(5, 4, 31 * s + 7, 1, 100) for s in range(1200)]
    out, refs = check(insts)
    assert all(r["status"] == sx.FEASIBLE for r in refs)
    assert out.evicted == 0


@pytest.mark.parametrize("n,m,B", [(4, 512, 3), (4, 513, 3), (500, 6, 2), (507, 6, 2)])
def test_workspace_class_and_tile_boundaries(gpu, n, m, B):
    """(4, 512) and (4, 513): the workspace class, 512 / 513 rows in the ratio argmin and the
    objective GEMV; (500, 6) and (507, 6): 512 / 513 entering candidates in phase 1 / phase 2"""
    assert sx.batch_class(n, m) == (1 if m >= 512 else 2)
    insts = [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in range(1, B + 1)]
    out, _ = check(insts)
    assert out.evicted == 0


def test_pivot_cap(gpu):
    inst = oracle.generate(10, 20, 8939, -100, 100)
    out, refs = check([inst], max_pivots=3)
    assert refs[0]["status"] == sx.PIVOT_CAP and refs[0]["pivots"] == (3, 0) and len(refs[0]["row"]) == 51
    assert out.status.tolist() == [sx.PIVOT_CAP] and out.row_width.tolist() == [51]


def test_eviction(gpu):
    """a resident budget of 2 pivots per phase: the kernel leaves the problems that need a third
    NOT_ENDED and counts them; finish=True re-solves them, so the results do not change"""
    n, m = 20, 10
    insts = [oracle.generate(n, m, seed, 1, 100) for seed in (2010, 3010, 4010, 5010)]
    refs = [ref_with_row(*abc) for abc in insts]
    assert refs[0]["pivots"][0] == 15
    A, b, c = tensors(insts)
    sx.set_batch_budget(2)
    try:
        raw = sx.solve_batch_tensors(A, b, c, objective_row=True, finish=False)
        torch.cuda.current_stream().synchronize()
        assert isinstance(raw.evicted, torch.Tensor) and raw.evicted.dtype == torch.int32
        left = raw.status == sx.NOT_ENDED
        assert int(raw.evicted.item()) == int(left.sum().item()) > 0
        # what the kernel leaves of an evicted problem: NaN, zeros, width 0
        assert torch.isnan(raw.optimal_value[left]).all()
        assert not raw.solution[left].view(torch.int64).any()
        assert not raw.objective_row[left].view(torch.int64).any()
        assert not raw.row_width[left].any()
        done = sx.solve_batch_tensors(A, b, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert done.evicted == int(left.sum().item())
    same_as_refs(done, refs, n, m)


def test_non_default_streams(gpu):
    """the launch goes on torch's current stream: one call on a side stream, then two calls on two
    streams with their own outputs, each correct after its stream is synchronised"""
    sets = [mixed(12, 9), [oracle.generate(20, 10, 1000 * s + 2010, 1, 100) for s in range(1, 9)]]
    dev = [tensors(insts) for insts in sets]
    refs = [[ref_with_row(*abc) for abc in insts] for insts in sets]
    shapes = [(12, 9), (20, 10)]
    torch.cuda.synchronize()  # the inputs are complete before any side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        out = sx.solve_batch_tensors(*dev[0], objective_row=True, finish=False)
    s0.synchronize()
    same_as_refs(out, refs[0], *shapes[0])
    assert int(out.evicted.item()) == 0

    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s, t in zip(streams, dev):
        with torch.cuda.stream(s):
            outs.append(sx.solve_batch_tensors(*t, objective_row=True, finish=False))
    for s in streams:
        s.synchronize()
    for o, r, (n, m) in zip(outs, refs, shapes):
        same_as_refs(o, r, n, m)


def test_empty_call(gpu):
    n, m = 20, 10
    A = torch.empty((0, m, n), dtype=torch.float64, device="cuda")
    b = torch.empty((0, m), dtype=torch.float64, device="cuda")
    c = torch.empty((0, n), dtype=torch.float64, device="cuda")
    out = sx.solve_batch_tensors(A, b, c, objective_row=True)
    assert out.evicted == 0
    assert out.status.shape == (0,) and out.pivots.shape == (0, 2) and out.optimal_value.shape == (0,)
    assert out.solution.shape == (0, n) and out.base.shape == (0, m)
    assert out.objective_row.shape == (0, 1 + n + 2 * m) and out.row_width.shape == (0,)
    assert all(t.is_cuda for t in (out.status, out.pivots, out.optimal_value, out.solution, out.base))


def test_agrees_with_solve_batch(gpu):
    insts = mixed(12, 9)
    out = sx.solve_batch_tensors(*tensors(insts))
    probs = [sx.Problem.from_arrays(*abc) for abc in insts]
    try:
        res = sx.solve_batch(probs)
    finally:
        for p in probs:
            p.close()
    status, pivots, opt = out.status.cpu().numpy(), out.pivots.cpu().numpy(), out.optimal_value.cpu().numpy()
    x, base = out.solution.cpu().numpy(), out.base.cpu().numpy()
    for k, r in enumerate(res):
        assert r.status == two_phase_ref(*insts[k])["status"]
        assert status[k] == r.status and tuple(pivots[k]) == tuple(r.pivots)
        assert np.array_equal(base[k], r.base)
        if r.status == sx.FEASIBLE:
            assert bits(opt[k]) == bits(r.optimal_value)
            assert np.array_equal(bits(x[k]), bits(r.solution))
