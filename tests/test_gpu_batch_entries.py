"""The three device batch entries write the same bytes (needs an MI355X).  k_batch_solve_dev and
k_batch_solve_st share one epilogue (sx_batch.hip wg_write_results), k_batch_solve_rag keeps the same
stores written out over its envelope; here the same instances go through all three --
solve_batch_tensors as it is, with n_active / m_active full (the ragged kernel) and with
keep_state=True (the state kernel) -- and every output tensor must agree bit for bit, the NaN pattern of optimal_value included: on every outcome, under a pivot cap,
and for evicted problems.  The outcome counts asserted below are the CPU oracle's."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
import test_gpu_batch_device as tbd
from batch_refs import ref_with_row, same_as_refs, same_tensors, tensors

pytestmark = pytest.mark.gpu


def three_entries(A, b, c, n, m, max_pivots=-1):
    """(one-shape, ragged, state) results of the same call, complete on return"""
    B = A.shape[0]
    full = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    kw = dict(max_pivots=max_pivots, objective_row=True, finish=False)
    outs = (sx.solve_batch_tensors(A, b, c, **kw),
            sx.solve_batch_tensors(A, b, c, n_active=full(n), m_active=full(m), **kw),
            sx.solve_batch_tensors(A, b, c, keep_state=True, **kw))
    torch.cuda.current_stream().synchronize()
    assert outs[1].n_active is not None and outs[2].state is not None and outs[0].state is None
    return outs


def same_bytes(outs):
    one, rag, st = outs
    for other in (rag, st):
        same_tensors(other, one)  # (float fields as int64 views: NaN bits and signed zeros count)
        assert int(other.evicted.item()) == int(one.evicted.item())
    return one


def outcome_counts(refs):
    counts = {}
    for r in refs:
        key = (r["status"], len(r["row"]))
        counts[key] = counts.get(key, 0) + 1
    return counts


def test_every_outcome_and_the_pivot_cap(gpu):
    n, m = 12, 9
    insts = tbd.mixed(n, m)
    A, b, c = tensors(insts)
    want = {-1: {(sx.FEASIBLE, 22): 3, (sx.UNBOUNDED, 22): 11, (sx.INFEASIBLE, 31): 10},
            12: {(sx.PIVOT_CAP, 31): 17, (sx.UNBOUNDED, 22): 3, (sx.INFEASIBLE, 31): 4}}
    for cap in (-1, 12):
        refs = [ref_with_row(*inst, max_pivots=cap) for inst in insts]
        assert outcome_counts(refs) == want[cap], cap
        one = same_bytes(three_entries(A, b, c, n, m, cap))
        assert int(one.evicted.item()) == 0
        one.evicted = 0
        same_as_refs(one, refs, n, m)


def test_evicted_problems(gpu):
    """a resident budget of 12 pivots per phase: the oracle's phase-1 counts are 8 to 20, so the
    problems that need a 13th pivot in a phase are evicted -- a zero row of width 0, a NaN objective
    and a zero solution from every entry -- and the others end as the oracle does"""
    n, m, budget = 12, 9, 12
    insts = tbd.mixed(n, m)
    refs = [ref_with_row(*inst) for inst in insts]
    p1 = [r["pivots"][0] for r in refs]
    assert (min(p1), max(p1)) == (8, 20) and sum(p > budget for p in p1) == 16
    left = [k for k, r in enumerate(refs) if max(r["pivots"]) > budget]
    assert len(left) == 16  # no problem is evicted in phase 2 alone
    A, b, c = tensors(insts)
    sx.set_batch_budget(budget)
    try:
        one = same_bytes(three_entries(A, b, c, n, m))
    finally:
        sx.set_batch_budget(0)
    assert int(one.evicted.item()) == 16
    assert torch.nonzero(one.status == sx.NOT_ENDED).flatten().tolist() == left
    assert not one.objective_row[left].view(torch.int64).any() and not one.row_width[left].any()
    assert not one.solution[left].view(torch.int64).any() and torch.isnan(one.optimal_value[left]).all()
    assert one.pivots[left].tolist() == [[budget, 0]] * 16
    keep = [k for k in range(len(insts)) if k not in left]
    done = sx.BatchTensors(one.status[keep], one.pivots[keep], one.optimal_value[keep], one.solution[keep], one.base[keep],
                           one.objective_row[keep], one.row_width[keep], 0)
    same_as_refs(done, [refs[k] for k in keep], n, m)


def test_workspace_class_under_a_cap(gpu):
    """(4, 513): the <false> kernels and their slices, two row tiles; capped after 2 pivots"""
    n, m, B = 4, 513, 3
    assert sx.batch_class(n, m) == 1
    insts = tbd.mixed(n, m)[:B]
    refs = [ref_with_row(*inst, max_pivots=2) for inst in insts]
    assert [(r["status"], r["pivots"]) for r in refs] == [(sx.PIVOT_CAP, (2, 0))] * B
    one = same_bytes(three_entries(*tensors(insts), n, m, 2))
    assert int(one.evicted.item()) == 0
    one.evicted = 0
    same_as_refs(one, refs, n, m)
    assert np.array_equal(one.row_width.cpu().numpy(), np.full(B, 1 + n + 2 * m, dtype=np.int32))
