"""A kept batch state grown by new structural columns (simplex_solve_batch_device_cols, sx_batch.hip
k_batch_solve_cols) through sx.add_cols_batch_tensors, and through a ctypes caller (device_entries.cols_call) for
what that never passes.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_cols_refs.py: the entry restated
from batch_rhs_refs' sums and dual loop, batch_state_refs._run and the oracle's gemv_partials
(test_batch_cols_host.py shows on the CPU what the restatement reaches, and which instances pivot).
Compared per problem: status, both pivot counts, the basis, objective and solution (NaN and zeros
unless FEASIBLE), the objective row and its width, and the whole grown state: T, d, base, phase and
pivots.  A kept state is the solve of the grown tensors' first n0 columns, a sliced view."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_cols_refs import (CAP_SHAPE, COLS_CAPS, KINDS, RESCUE_SHAPES, append_column, cols_shapes, elastic, kept_part,
                             many_grown, ref_cols, want_batch)
from batch_refs import same_as_refs, same_tensors, tensors
from batch_rhs_refs import negated_rhs, ref_rhs, ref_rhs_resume, scaled_rhs
from batch_rows_refs import grow, ref_rows
from batch_state_refs import (bits, mixed_instances, ref_state, same_as_state_refs, save_instances, state_tensors)
from device_entries import cols_call, dense

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")


def kept(grown, n0, max_pivots=-1):
    """one keep_state call on the first n0 columns of the grown tensors, checked against the
    reference: (BatchTensors, refs)"""
    A, b, c = tensors(grown)
    out = sx.solve_batch_tensors(A[:, :, :n0], b, c[:, :n0], max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*kept_part(g, n0), max_pivots) for g in grown]
    same_as_state_refs(out, refs, n0, A.shape[1])
    return out, refs


def add(state, grown, **kw):
    """the columns of `grown` (instances in the grown shape) added to `state`"""
    A, b, c = tensors(grown)
    out = sx.add_cols_batch_tensors(state, A, b, c, objective_row=True, **kw)
    m, n = grown[0][0].shape
    assert out.state is not state and out.state.rhs is True and (out.state.n, out.state.m) == (n, m)
    return out


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m, state.rhs)


def same_state(x, y):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in ("base", "phase", "pivots"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f


def dev(rows):
    return torch.from_numpy(np.stack(rows)).cuda()


# ------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("n0,p,m", cols_shapes())
def test_shapes(gpu, n0, p, m):
    """a column that does not price in (no pivot), one that does (phase 2 pivots) and a non-positive
    column with a positive cost (UNBOUNDED), on every shape: the in-state's dense stride 1 + n0 + m in
    both parities, p = 3, the LDS class, the workspace class and the step from one to the other, the
    leaving ratio over two row tiles, the new column last in the first entering tile and first in the
    second"""
    first = keep = None
    for kind, theta in KINDS:
        _, grown, refs, want = want_batch(n0, p, m, kind, theta)
        if first is None:
            first, _ = kept(grown, n0)
            keep = clone(first.state)
        assert not any(w["cold"] for w in want)
        assert all(w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
        out = add(first.state, grown)
        assert out.evicted == 0
        same_as_state_refs(out, want, n0 + p, m)
    same_state(first.state, keep)


# ------------------------------------------------------------------ cold and warm in one batch
def test_mixed_states(gpu):
    """phase-1 (INFEASIBLE), UNBOUNDED and FEASIBLE states in one call: the phase-1 ones are cold,
    solve_batch_tensors on the grown problem; an UNBOUNDED one simply continues"""
    insts = mixed_instances()
    m, n0 = insts[0][0].shape
    grown = [(np.hstack([A, np.ones((m, 1))]), b, np.append(c, 50.0)) for A, b, c in insts]
    first, refs = kept(grown, n0)
    want = [ref_cols(r, *g) for r, g in zip(refs, grown)]
    cold = [k for k, w in enumerate(want) if w["cold"]]
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold} == {(1, sx.INFEASIBLE)}
    assert {r["status"] for r in refs} >= {sx.INFEASIBLE, sx.UNBOUNDED, sx.FEASIBLE}
    assert 0 < len(cold) < len(insts)
    out = add(first.state, grown)
    same_as_state_refs(out, want, n0 + 1, m)
    plain = sx.solve_batch_tensors(*tensors(grown), objective_row=True)
    pick = lambda o: sx.BatchTensors(*(t[cold] for t in (o.status, o.pivots, o.optimal_value, o.solution, o.base,  # noqa: E731
                                                          o.objective_row, o.row_width)), 0)
    same_tensors(pick(out), pick(plain))


# ------------------------------------------------------------------ phase-3 rescue
@pytest.mark.parametrize("n,m", RESCUE_SHAPES)
def test_elastic_column_rescues_a_phase_3_state(gpu, n, m):
    """states left INFEASIBLE inside the dual loop by a re-rhs with b_0 negated: an elastic column (-1 in
    row 0) with cost -1000 is warm -- one dual pivot, FEASIBLE --, the same column with cost +1 prices
    in, so the problem is cold"""
    insts = save_instances(n, m)
    first, refs = kept(insts, n)
    A, b, c = tensors(insts)
    b2s = [negated_rhs(inst[1], 0) for inst in insts]
    stuck_refs = [ref_rhs(r, inst[0], b2, inst[2]) for r, inst, b2 in zip(refs, insts, b2s)]
    assert all(r["status"] == sx.INFEASIBLE and r["phase"] == 3 for r in stuck_refs)
    stuck = sx.resume_batch_tensors(first.state, c, objective_row=True, in_place=False, A=A, b=dev(b2s))
    same_as_state_refs(stuck, stuck_refs, n, m)
    for cost, is_cold in ((-1000.0, False), (1.0, True)):
        grown = [elastic((inst[0], b2, inst[2]), cost) for inst, b2 in zip(insts, b2s)]
        want = [ref_cols(r, *g) for r, g in zip(stuck_refs, grown)]
        assert all(w["cold"] == is_cold for w in want)
        if not is_cold:
            assert all(w["dual"] == 1 and w["status"] == sx.FEASIBLE and w["phase"] == 2 for w in want)
        same_as_state_refs(add(stuck.state, grown), want, n + 1, m)


# ------------------------------------------------------------------ cap, budget
@pytest.mark.parametrize("cap", COLS_CAPS)
def test_cap_inside_the_warm_phase_2_and_resume(gpu, cap):
    n0, p, m = CAP_SHAPE
    _, grown, refs, whole = want_batch(n0, p, m, "scaled", 100.0)
    crefs = want_batch(n0, p, m, "scaled", 100.0, cap)[3]
    capped_ones = [k for k, w in enumerate(whole) if w["pivots"][1] > cap]
    assert len(capped_ones) >= 2
    assert all((crefs[k]["status"], crefs[k]["phase"], crefs[k]["pivots"][1]) == (sx.PIVOT_CAP, 2, cap) for k in capped_ones)
    first, _ = kept(grown, n0)
    capped = add(first.state, grown, max_pivots=cap)
    same_as_state_refs(capped, crefs, n0 + p, m)
    c = tensors(grown)[2]
    keep = clone(capped.state)
    done = sx.resume_batch_tensors(capped.state, c, objective_row=True, in_place=False)
    assert done.state.rhs is True and done.evicted == 0
    same_as_state_refs(done, whole, n0 + p, m)
    same_state(capped.state, keep)


def test_budget_inside_the_warm_phase_2(gpu):
    """a resident budget of 2 pivots per call: evicted inside phase 2 with the state a cap of 2 leaves,
    and every plain resume takes it 2 pivots further, until nothing is evicted"""
    n0, p, m = CAP_SHAPE
    _, grown, refs, whole = want_batch(n0, p, m, "scaled", 100.0)
    cap2 = want_batch(n0, p, m, "scaled", 100.0, 2)[3]
    assert all(w["pivots"][1] > 2 for w in whole)
    first, _ = kept(grown, n0)
    c = tensors(grown)[2]
    bound = max(w["pivots"][1] for w in whole) // 2 + 2
    sx.set_batch_budget(2)
    try:
        out = add(first.state, grown)
        assert out.evicted == 3 and out.status.tolist() == [sx.NOT_ENDED] * 3
        assert out.state.phase.tolist() == [2] * 3 and out.pivots[:, 1].tolist() == [2] * 3
        same_state(out.state, state_tensors(cap2))
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= bound, "an evicted problem does not progress"
            out = sx.resume_batch_tensors(out.state, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= min(w["pivots"][1] for w in whole) // 2 - 1
    same_as_state_refs(out, whole, n0 + p, m)


# ------------------------------------------------------------------ chains
def test_column_then_row_then_new_rhs_then_column(gpu):
    """the grown state is a state of the rows entry and of the right-hand-side entry, and theirs are
    states of this one"""
    n0, p, m = 20, 1, 10
    _, grown, refs, want = want_batch(n0, p, m, "scaled", 100.0)
    first, _ = kept(grown, n0)
    one = add(first.state, grown)
    same_as_state_refs(one, want, n0 + 1, m)
    assert all(w["status"] == sx.FEASIBLE for w in want)
    grown2 = [grow(g, ["cut"], 0.5) for g in grown]
    want2 = [ref_rows(w, *g) for w, g in zip(want, grown2)]
    assert any(w["dual"] >= 1 for w in want2)
    A2, b2, c2 = tensors(grown2)
    two = sx.add_rows_batch_tensors(one.state, A2, b2, c2, objective_row=True)
    same_as_state_refs(two, want2, n0 + 1, m + 1)
    b3s = [scaled_rhs(g[1], 1000 + k, 0.3) for k, g in enumerate(grown2)]
    want3 = [ref_rhs(w, g[0], b3, g[2]) for w, g, b3 in zip(want2, grown2, b3s)]
    three = sx.resume_batch_tensors(two.state, c2, objective_row=True, in_place=False, A=A2, b=dev(b3s))
    same_as_state_refs(three, want3, n0 + 1, m + 1)
    grown4 = [append_column((g[0], b3, g[2]), 500 + k, 100.0) for k, (g, b3) in enumerate(zip(grown2, b3s))]
    want4 = [ref_cols(w, *g) for w, g in zip(want3, grown4)]
    assert any(w["pivots"][1] >= 1 and not w["cold"] for w in want4)
    same_as_state_refs(add(three.state, grown4), want4, n0 + 2, m + 1)


def test_columns_on_a_state_grown_by_rows(gpu):
    n, m0 = 20, 10
    insts = save_instances(n, m0)
    first, refs = kept(insts, n)
    grown = [grow(inst, ["cut"], 0.5) for inst in insts]
    want = [ref_rows(r, *g) for r, g in zip(refs, grown)]
    A, b, c = tensors(grown)
    one = sx.add_rows_batch_tensors(first.state, A, b, c, objective_row=True)
    same_as_state_refs(one, want, n, m0 + 1)
    grown2 = [append_column(append_column(g, 600 + k, 100.0), 700 + k, 100.0) for k, g in enumerate(grown)]
    want2 = [ref_cols(w, *g) for w, g in zip(want, grown2)]
    assert any(w["pivots"][1] >= 1 for w in want2) and not any(w["cold"] for w in want2)
    same_as_state_refs(add(one.state, grown2), want2, n + 2, m0 + 1)


# ------------------------------------------------------------------ strides, many problems, a stream
def test_strided_c_and_transposed_a(gpu):
    n0, p, m = 20, 1, 10
    n = n0 + p
    _, grown, refs, want = want_batch(n0, p, m, "scaled", 100.0)
    first, _ = kept(grown, n0)
    A, b, c = tensors(grown)
    wide = torch.full((len(grown), 2 * n + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * n + 1:2] = c
    view = wide[:, 1:2 * n + 1:2]
    assert view.stride() == (2 * n + 3, 2)
    At = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert At.stride() == (n * m, 1, m)
    out = sx.add_cols_batch_tensors(first.state, At, b, view, objective_row=True)
    same_as_state_refs(out, want, n, m)
    # the cold path reads A and c through their strides too
    cold = state_tensors([ref_state(*kept_part(g, n0), 2) for g in grown])
    assert cold.phase.tolist() == [1] * 3
    out = sx.add_cols_batch_tensors(cold, At, b, view, objective_row=True)
    same_as_state_refs(out, [ref_state(*g) for g in grown], n, m)


def test_more_problems_than_resident_workgroups(gpu):
    grown = many_grown()
    assert len(grown) == 1200
    first, refs = kept(grown, 5)
    want = [ref_cols(r, *g) for r, g in zip(refs, grown)]
    assert sum(w["pivots"][1] >= 1 for w in want) >= 100
    same_as_state_refs(add(first.state, grown), want, 6, 4)


def test_non_default_stream(gpu):
    n0, p, m = CAP_SHAPE
    _, grown, refs, whole = want_batch(n0, p, m, "scaled", 100.0)
    first, _ = kept(grown, n0)
    A, b, c = tensors(grown)
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.add_cols_batch_tensors(first.state, A, b, c, max_pivots=2, objective_row=True, finish=False)
        done = sx.resume_batch_tensors(capped.state, c, objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, want_batch(n0, p, m, "scaled", 100.0, 2)[3], n0 + p, m)
    same_as_state_refs(done, whole, n0 + p, m)


# ------------------------------------------------------------------ bad states
def test_bad_states(gpu):
    """a base entry that the grown shape would accept but the in-state's does not, phase 0 and a
    negative pivot count: BAD_STATE, cleared outputs and phase 0 for that problem alone"""
    n0, p, m = 20, 1, 10
    _, grown3, _, _ = want_batch(n0, p, m, "scaled", 100.0)
    grown = grown3 + grown3[:1]
    first, refs = kept(grown, n0)
    state = clone(first.state)
    state.base[0, 3] = n0 + m       # < n0 + 1 + m: the grown shape's last slack, not a variable of the in-state
    state.phase[1] = 0
    state.pivots[2, 1] = -1
    out = add(state, grown)
    bad = [0, 1, 2]
    assert out.status.tolist() == [sx.BAD_STATE] * 3 + [sx.FEASIBLE]
    assert out.state.phase.tolist() == [0] * 3 + [2] and not out.pivots[bad].any()
    assert torch.isnan(out.optimal_value[bad]).all() and not out.solution[bad].view(torch.int64).any()
    assert (out.base[bad] == -1).all() and not out.objective_row[bad].view(torch.int64).any()
    assert not out.row_width[bad].any()
    good = sx.BatchTensors(*(t[3:] for t in (out.status, out.pivots, out.optimal_value, out.solution, out.base,
                                              out.objective_row, out.row_width)), 0)
    same_as_refs(good, [ref_cols(refs[3], *grown[3])], n0 + p, m)


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: `out` NULL and every optional output NULL; then into a state with the outputs"""
    n0, p, m = CAP_SHAPE
    n = n0 + p
    _, grown, refs, whole = want_batch(n0, p, m, "scaled", 100.0)
    B = len(grown)
    first, _ = kept(grown, n0)
    A, b, c = tensors(grown)
    keep = clone(first.state)
    o = cols_call(n, m, B, dense(A), dense(b), dense(c), first.state, p, x=None, base=None, objrow=None, row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(first.state, keep)  # nothing was written to `in`
    assert o.status.tolist() == [r["status"] for r in whole]
    assert [tuple(q) for q in o.pivots.tolist()] == [r["pivots"] for r in whole]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([r["opt"] for r in whole]))
    assert int(o.evicted.item()) == 0
    capped = sx.BatchState.empty(B, n, m, "cuda")
    o = cols_call(n, m, B, dense(A), dense(b), dense(c), first.state, p, state_out=capped, max_pivots=2)
    assert o.rc == 0 and o.status.tolist() == [sx.PIVOT_CAP] * B
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, capped)
    crefs = want_batch(n0, p, m, "scaled", 100.0, 2)[3]
    same_as_state_refs(got, crefs, n, m)
    capped.rhs = True
    done = sx.resume_batch_tensors(capped, c, objective_row=True)
    same_as_state_refs(done, [ref_rhs_resume(r, g[2]) for r, g in zip(crefs, grown)], n, m)
    same_as_state_refs(done, whole, n, m)
