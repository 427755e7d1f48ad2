"""What the GPU tests of the batched solve share (test_gpu_batch_device.py, test_gpu_batch_ladders.py):
the oracle's result with its objective row, computed once per instance, and the bit-for-bit
comparison of a solve_batch_tensors result with it:

  always                       status, both pivot counts, the basis
  FEASIBLE                     objective and solution as uint64 bit patterns
  otherwise                    the solution is all +0.0 and the objective a NaN
  with objective_row=True      row_width == len(oracle row), the row's bits, +0.0 behind row_width
"""
import numpy as np
import torch

import oracle
import simplexoncuda_amd as sx

_REF = {}


def ref_with_row(A, b, c, max_pivots=-1):
    """oracle.two_phase plus its final objective row (two_phase_ref's cache does not keep the row);
    computed once per instance and cap"""
    key = (A.tobytes(), b.tobytes(), c.tobytes(), A.shape, max_pivots)
    if key not in _REF:
        r = oracle.two_phase(A, b, c, max_pivots)
        r["row"] = oracle.last_objective_row().copy()
        _REF[key] = r
    return _REF[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tensors(insts):
    """[(A m x n, b, c)] of one shape -> contiguous device tensors A [B, m, n], b [B, m], c [B, n]"""
    return tuple(torch.from_numpy(np.stack([inst[k] for inst in insts])).cuda() for k in range(3))


def same_as_refs(out, refs, n, m):
    """every field of a BatchTensors against the oracle's results (with "row" when the call asked
    for the objective row)"""
    B = len(refs)
    N1 = 1 + n + 2 * m
    status, pivots, opt = out.status.cpu().numpy(), out.pivots.cpu().numpy(), out.optimal_value.cpu().numpy()
    x, base = out.solution.cpu().numpy(), out.base.cpu().numpy()
    assert status.shape == (B,) and status.dtype == np.int32
    assert pivots.shape == (B, 2) and pivots.dtype == np.int64
    assert opt.shape == (B,) and x.shape == (B, n) and base.shape == (B, m) and base.dtype == np.int32
    rows = widths = None
    if out.objective_row is not None:
        rows, widths = out.objective_row.cpu().numpy(), out.row_width.cpu().numpy()
        assert rows.shape == (B, N1) and widths.shape == (B,) and widths.dtype == np.int32
    for k, ref in enumerate(refs):
        assert status[k] == ref["status"], k
        assert tuple(pivots[k]) == ref["pivots"], k
        assert np.array_equal(base[k], ref["base"]), k
        if ref["status"] == sx.FEASIBLE:
            assert bits(opt[k]) == bits(ref["opt"]), k
            assert np.array_equal(bits(x[k]), bits(ref["x"])), k
        else:
            assert np.isnan(opt[k]), k
            assert not bits(x[k]).any(), k
        if rows is not None:
            w = len(ref["row"])
            assert widths[k] == w and w in (1 + n + m, N1), k
            assert np.array_equal(bits(rows[k, :w]), bits(ref["row"])), k
            assert not bits(rows[k, w:]).any(), k


def same_tensors(x, y):
    for f in ("status", "pivots", "base", "row_width"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("optimal_value", "solution", "objective_row"):  # bit patterns: NaN == NaN, -0.0 != +0.0
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f
    assert x.evicted == y.evicted
