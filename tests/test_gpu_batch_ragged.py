"""Ragged device batch (simplex_solve_batch_device_ragged, sx_batch.hip k_batch_solve_rag) through
sx.solve_batch_tensors(..., n_active=, m_active=, order=): per-problem shapes inside one padded
envelope (needs an MI355X).  Every problem of every call is compared with the CPU oracle's result
for ITS OWN n_k x m_k sub-problem, computed at test time (batch_refs.ref_with_row), bit for bit and
without a tolerance, in the envelope's conventions (same_as_ragged_refs):

  always                       status, both pivot counts, base[:m_k] in the problem's numbering, base[m_k:] == -1
  FEASIBLE                     objective and solution[:n_k] as uint64 bit patterns, solution[n_k:] +0.0
  otherwise                    the solution is all +0.0 and the objective a NaN
  with objective_row=True      row_width == len(oracle row); the row in envelope columns: [0], structural
                               entries at [1 + j], slack entries at [1 + n + i], artificial entries at
                               [1 + n + m + i], +0.0 in every other entry
  BAD_SHAPE (ref None)         pivots 0, objective NaN, solution and row +0.0, base -1, row_width 0

Unless a test says otherwise the inputs outside the active blocks are NaN, and all three input tensors
are compared with clones after the call: nothing outside a problem's block is read (a NaN would
reach some result) and no input is written."""
import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
import tie_ladders as tl
from batch_refs import bits, ref_with_row, same_tensors

pytestmark = pytest.mark.gpu


def envelope(insts, n, m, fill=float("nan")):
    """[(A m_k x n_k, b, c)] -> contiguous device tensors A [B, m, n], b [B, m], c [B, n] with every
    problem in the leading block of its slot and `fill` elsewhere, and the int32 dimension tensors"""
    B = len(insts)
    A, b, c = np.full((B, m, n), fill), np.full((B, m), fill), np.full((B, n), fill)
    for k, (Ak, bk, ck) in enumerate(insts):
        mk, nk = Ak.shape
        A[k, :mk, :nk], b[k, :mk], c[k, :nk] = Ak, bk, ck
    n_k = torch.tensor([inst[0].shape[1] for inst in insts], dtype=torch.int32).cuda()
    m_k = torch.tensor([inst[0].shape[0] for inst in insts], dtype=torch.int32).cuda()
    return tuple(torch.from_numpy(t).cuda() for t in (A, b, c)), n_k, m_k


def envelope_row(d, nk, mk, n, m):
    """a problem's logical objective row (1 + nk + mk or 1 + nk + 2 mk entries) in envelope columns"""
    e = np.zeros(1 + n + 2 * m)
    e[:1 + nk] = d[:1 + nk]
    e[1 + n:1 + n + mk] = d[1 + nk:1 + nk + mk]
    art = d[1 + nk + mk:]
    assert len(art) in (0, mk)
    e[1 + n + m:1 + n + m + len(art)] = art
    return e


def same_as_ragged_refs(out, refs, dims, n, m):
    """every field of a ragged BatchTensors against the oracle's results of the sub-problems (with
    "row" when the call asked for the objective row); refs[k] None: problem k must be BAD_SHAPE"""
    B = len(refs)
    N1 = 1 + n + 2 * m
    status, pivots, opt = out.status.cpu().numpy(), out.pivots.cpu().numpy(), out.optimal_value.cpu().numpy()
    x, base = out.solution.cpu().numpy(), out.base.cpu().numpy()
    assert status.shape == (B,) and status.dtype == np.int32
    assert pivots.shape == (B, 2) and pivots.dtype == np.int64
    assert opt.shape == (B,) and x.shape == (B, n) and base.shape == (B, m) and base.dtype == np.int32
    assert out.n_active.tolist() == [d[0] for d in dims] and out.m_active.tolist() == [d[1] for d in dims]
    rows = widths = None
    if out.objective_row is not None:
        rows, widths = out.objective_row.cpu().numpy(), out.row_width.cpu().numpy()
        assert rows.shape == (B, N1) and widths.shape == (B,) and widths.dtype == np.int32
        assert out.duals.shape == (B, m) and out.reduced_costs.shape == (B, n)
    for k, (ref, (nk, mk)) in enumerate(zip(refs, dims)):
        if ref is None:
            assert status[k] == sx.BAD_SHAPE and tuple(pivots[k]) == (0, 0) and np.isnan(opt[k]), k
            assert not bits(x[k]).any() and (base[k] == -1).all(), k
            if rows is not None:
                assert widths[k] == 0 and not bits(rows[k]).any(), k
            continue
        assert status[k] == ref["status"], k
        assert tuple(pivots[k]) == ref["pivots"], k
        assert np.array_equal(base[k, :mk], ref["base"]) and (base[k, mk:] == -1).all(), k
        if ref["status"] == sx.FEASIBLE:
            assert bits(opt[k]) == bits(ref["opt"]), k
            assert np.array_equal(bits(x[k, :nk]), bits(ref["x"])), k
            assert not bits(x[k, nk:]).any(), k
        else:
            assert np.isnan(opt[k]), k
            assert not bits(x[k]).any(), k
        if rows is not None:
            w = len(ref["row"])
            assert widths[k] == w and w in (1 + nk + mk, 1 + nk + 2 * mk), k
            assert np.array_equal(bits(rows[k]), bits(envelope_row(ref["row"], nk, mk, n, m))), k
            if ref["status"] == sx.FEASIBLE:  # the views hold the problem's duals and reduced costs
                assert np.array_equal(bits(out.duals[k, :mk].cpu().numpy()), bits(ref["row"][1 + nk:1 + nk + mk])), k
                assert np.array_equal(bits(out.reduced_costs[k, :nk].cpu().numpy()), bits(ref["row"][1:1 + nk])), k


def check(insts, n, m, max_pivots=-1, objective_row=True, **kw):
    """one ragged call over a NaN-padded envelope; the inputs must come back unchanged; returns
    (BatchTensors, oracle results)"""
    (A, b, c), n_k, m_k = envelope(insts, n, m)
    keep = [t.clone() for t in (A, b, c, n_k, m_k)]
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=objective_row, n_active=n_k,
                                 m_active=m_k, **kw)
    assert all(torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t,
                           k.view(torch.int64) if k.dtype == torch.float64 else k)
               for t, k in zip((A, b, c, n_k, m_k), keep))
    refs = [ref_with_row(*abc, max_pivots=max_pivots) for abc in insts]
    same_as_ragged_refs(out, refs, [(inst[0].shape[1], inst[0].shape[0]) for inst in insts], n, m)
    return out, refs


def gen(n, m, s, lo=1, hi=100):
    return oracle.generate(n, m, (1000 if lo == 1 else 7919) * s + n * 100 + m, lo, hi)


# ------------------------------------------------------------------ 1. uniform dims
@pytest.mark.parametrize("n,m,B", [(20, 10, 5), (4, 513, 3)])
def test_uniform_dims_equal_the_one_shape_entry(gpu, n, m, B):
    """every block fully active (no NaN anywhere): byte for byte the one-shape entry's tensors, in
    the LDS class and in the workspace class; with one of the two dimensions left to the envelope too"""
    assert sx.batch_class(n, m) == (2 if m < 512 else 1)
    insts = [gen(n, m, s) for s in range(1, B + 1)]
    (A, b, c), n_k, m_k = envelope(insts, n, m)
    want = sx.solve_batch_tensors(A, b, c, objective_row=True)
    assert want.n_active is None and want.m_active is None
    for kw in ({"n_active": n_k, "m_active": m_k}, {"n_active": n_k}, {"m_active": m_k}):
        got = sx.solve_batch_tensors(A, b, c, objective_row=True, **kw)
        same_tensors(got, want)
        assert got.n_active.tolist() == [n] * B and got.m_active.tolist() == [m] * B


# ------------------------------------------------------------------ 2. mixed shapes
# the smallest and the envelope-filling shapes in each direction, two ordinary ones, and the row
# update's lane groups at 1 + n + m = 16 | 17 and 32 | 33
_MIXED_SHAPES = [(1, 1), (33, 33), (33, 1), (1, 33), (5, 4), (20, 10), (7, 8), (8, 8), (15, 16), (16, 16)]


def _mixed_insts():
    assert [1 + n + m for n, m in _MIXED_SHAPES[6:]] == [16, 17, 32, 33]
    return [gen(n, m, s, lo, hi) for n, m in _MIXED_SHAPES for lo, hi in ((1, 100), (-100, 100)) for s in (1, 2, 3)]


@pytest.mark.parametrize("objective_row", [True, False])
def test_mixed_shapes_in_one_envelope(gpu, objective_row):
    insts = _mixed_insts()
    out, refs = check(insts, 33, 33, objective_row=objective_row)
    assert {r["status"] for r in refs} >= {sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED}
    widths = {len(r["row"]) - (1 + inst[0].shape[1] + inst[0].shape[0]) == 0 for r, inst in zip(refs, insts)}
    assert widths == {True, False}  # phase-2 rows (1 + n_k + m_k) and phase-1 rows (1 + n_k + 2 m_k)
    assert out.evicted == 0
    assert (out.objective_row is None) == (not objective_row) and (out.row_width is None) == (not objective_row)


# ------------------------------------------------------------------ 3. tile boundaries
@pytest.mark.parametrize("n,m,actives", [
    (4, 513, [(4, 512), (4, 513), (1, 1), (2, 3)]),      # 512 | 513 ratio rows, workspace class
    (507, 6, [(500, 6), (501, 6), (507, 6), (1, 6)]),    # n + 2m = 512 | 513 entering candidates
])
def test_tile_boundaries_inside_a_larger_envelope(gpu, n, m, actives):
    assert sx.batch_class(n, m) == (1 if m >= 512 else 2)
    out, _ = check([gen(nk, mk, 1) for nk, mk in actives], n, m)
    assert out.evicted == 0


# ------------------------------------------------------------------ 4. a tie-ladder LP as a sub-problem
_LADDER_ENV = (48, 72)


def _ladder_insts():
    n, m, _ = tl.BATCH_CASES["B-small"][1]
    assert (n, m) == (40, 60) and n < _LADDER_ENV[0] and m < _LADDER_ENV[1]
    return [gen(20, 10, 1), tl.make_batch("B-small"), gen(48, 72, 1, -100, 100)]


@pytest.mark.parametrize("cap", [-1, 1, 8, 40])
def test_tie_ladder_as_a_sub_problem(gpu, cap):
    """B-small (40 x 60; tests/test_tie_ladders.py: the lane tree decides pivots of both phases) in a
    wider and taller envelope beside two other shapes: the whole solve and capped prefixes.  An
    argmin over the envelope's lengths, not the problem's, would run another tree"""
    insts = _ladder_insts()
    out, refs = check(insts, *_LADDER_ENV, max_pivots=cap)
    if cap < 0:
        assert (refs[1]["status"], refs[1]["pivots"]) == (sx.FEASIBLE, tl.BATCH_CASES["B-small"][5])
    else:
        assert (refs[1]["status"], refs[1]["pivots"], len(refs[1]["row"])) == (sx.PIVOT_CAP, (cap, 0), 1 + 40 + 120)
    assert out.evicted == 0


# ------------------------------------------------------------------ 5. more problems than workgroups
def test_more_problems_than_resident_workgroups(gpu):
    """1,200 problems in a (5, 4) envelope, the dimensions cycling through all 20 (n_k, m_k) pairs:
    a workgroup re-carves its working set for every problem it takes"""
    pairs = [(nk, mk) for nk in range(1, 6) for mk in range(1, 5)]
    insts = [oracle.generate(*pairs[s % 20], 31 * s + 7, 1, 100) for s in range(1200)]
    out, _ = check(insts, 5, 4)
    assert out.evicted == 0


# ------------------------------------------------------------------ 6. order
def test_results_do_not_depend_on_the_order(gpu):
    insts = _mixed_insts()
    B = len(insts)
    (A, b, c), n_k, m_k = envelope(insts, 33, 33)
    want, _ = check(insts, 33, 33, order=False)
    rng = np.random.default_rng(5)
    orders = [None, torch.arange(B - 1, -1, -1, dtype=torch.int32).cuda(),
              torch.from_numpy(rng.permutation(B).astype(np.int32)).cuda()]
    for order in orders:
        keep = None if order is None else order.clone()
        got = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k, order=order)
        same_tensors(got, want)
        assert order is None or torch.equal(order, keep)


# ------------------------------------------------------------------ 7. bad dims
def test_bad_dimensions_get_bad_shape(gpu):
    """dimensions just outside [1, n] x [1, m] between valid problems: BAD_SHAPE and cleared outputs
    for them (tested before anything is indexed with them), the oracle's results for the neighbours"""
    n, m = 6, 5
    bad = [(0, 3), (3, 0), (-1, 2), (n + 1, m), (n, m + 1)]
    good = [gen(nk, mk, 1) for nk, mk in [(6, 5), (3, 2), (1, 5), (6, 1), (2, 3), (4, 4)]]
    dims, refs, insts = [], [], []
    for k, inst in enumerate(good):
        insts.append(inst)
        dims.append((inst[0].shape[1], inst[0].shape[0]))
        refs.append(ref_with_row(*inst))
        if k < len(bad):
            insts.append((np.zeros((0, 0)), np.zeros(0), np.zeros(0)))  # (a slot that is all NaN)
            dims.append(bad[k])
            refs.append(None)
    (A, b, c), _, _ = envelope(insts, n, m)
    n_k = torch.tensor([d[0] for d in dims], dtype=torch.int32).cuda()
    m_k = torch.tensor([d[1] for d in dims], dtype=torch.int32).cuda()
    keep = [t.clone() for t in (A, b, c)]
    for order in (None, False):
        out = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k, order=order)
        same_as_ragged_refs(out, refs, dims, n, m)
        assert out.evicted == 0
        assert [sx.STATUS_NAMES[s] for s in out.status.tolist()].count("BAD_SHAPE") == len(bad)
    assert all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip((A, b, c), keep))


# ------------------------------------------------------------------ 8. eviction
def test_eviction(gpu):
    """a resident budget of 2 pivots per phase: the kernel leaves the problems that need a third
    NOT_ENDED, cleared, and counts them; finish=True re-solves them from their active blocks and
    writes them back in the ragged conventions"""
    insts = [gen(20, 10, 1), gen(1, 1, 1), gen(12, 9, 2, -100, 100), gen(33, 33, 1), gen(5, 4, 1), gen(8, 8, 3)]
    n, m = 33, 33
    (A, b, c), n_k, m_k = envelope(insts, n, m)
    refs = [ref_with_row(*abc) for abc in insts]
    dims = [(inst[0].shape[1], inst[0].shape[0]) for inst in insts]
    sx.set_batch_budget(2)
    try:
        raw = sx.solve_batch_tensors(A, b, c, objective_row=True, finish=False, n_active=n_k, m_active=m_k)
        torch.cuda.current_stream().synchronize()
        assert isinstance(raw.evicted, torch.Tensor) and raw.evicted.dtype == torch.int32
        left = raw.status == sx.NOT_ENDED
        assert left.tolist() == [max(r["pivots"]) > 2 for r in refs]
        assert int(raw.evicted.item()) == int(left.sum().item()) > 0 and not left.all()
        assert torch.isnan(raw.optimal_value[left]).all()
        assert not raw.solution[left].view(torch.int64).any()
        assert not raw.objective_row[left].view(torch.int64).any()
        assert not raw.row_width[left].any()
        done = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k)
    finally:
        sx.set_batch_budget(0)
    assert done.evicted == int(left.sum().item())
    same_as_ragged_refs(done, refs, dims, n, m)


# ------------------------------------------------------------------ 9. strided envelope
def test_strided_envelope(gpu):
    """a transposed view (the build walks A the other way) and a batch stride that is not the dense
    one, with ragged dimensions: the contiguous call's tensors, and nothing written"""
    insts = _mixed_insts()[::3]
    n, m, B = 33, 33, len(_mixed_insts()[::3])
    (A, b, c), n_k, m_k = envelope(insts, n, m)
    want, _ = check(insts, n, m)
    kw = dict(objective_row=True, n_active=n_k, m_active=m_k)

    At = A.transpose(1, 2).contiguous()
    keep = At.clone()
    view = At.transpose(1, 2)
    assert view.shape == A.shape and view.stride() == (n * m, 1, m)
    same_tensors(sx.solve_batch_tensors(view, b, c, **kw), want)
    assert torch.equal(At.view(torch.int64), keep.view(torch.int64))

    A2, b2, c2 = (torch.full((2 * B,) + tuple(t.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
                  for t in (A, b, c))
    A2[::2], b2[::2], c2[::2] = A, b, c
    keep = [t.clone() for t in (A2, b2, c2)]
    assert A2[::2].stride() == (2 * n * m, n, 1) and b2[::2].stride() == (2 * m, 1)
    same_tensors(sx.solve_batch_tensors(A2[::2], b2[::2], c2[::2], **kw), want)
    assert all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip((A2, b2, c2), keep))
