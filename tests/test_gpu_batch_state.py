"""The batch state (simplex_solve_batch_device_state, sx_batch.hip k_batch_solve_st) through
sx.solve_batch_tensors(keep_state=True) and sx.resume_batch_tensors, and through a ctypes caller
(device_entries.state_call) for what those never pass.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_state_refs.py: the state
restated from the oracle's build_phase1, update_objective and solve (test_batch_state_host.py shows
on the CPU that the restatement is oracle.two_phase, that a capped solve resumed is the whole solve,
and what the warm start reaches).  Compared per problem: status, both pivot counts, the basis,
objective and solution (NaN and zeros unless FEASIBLE), the objective row and its width, and the
saved T, d, base, phase and pivots."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
import structured_lps as slp
import tie_ladders as tl
from batch_refs import ref_with_row, same_as_refs, same_tensors, tensors
from batch_state_refs import (BAD_STATE_PHASE1_CAP, CAP_SHAPES, CAPS, LADDER_CAPS, MANY_CAP, SAVE_SHAPES,
                              STRUCTURED_FIRST_CAP, WARM_SCALES, WARM_SEEDS, WARM_SHAPES, bad_state_instances, bits,
                              cap_instances, cap_value, eviction_instances, ladder_instances, many_instances,
                              mixed_instances, ref_resume, ref_state, same_as_state_refs, save_instances,
                              state_tensors, structured_instances, warm_costs, warm_instances)
from device_entries import SENTINEL, dense, state_call

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")


def shape_of(insts):
    m, n = insts[0][0].shape
    return n, m


def fresh(insts, max_pivots=-1):
    """one keep_state call with the objective row, checked against the reference: (BatchTensors, refs, c)"""
    A, b, c = tensors(insts)
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, *shape_of(insts))
    return out, refs, c


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m)


def same_state(x, y):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in ("base", "phase", "pivots"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f


# ------------------------------------------------------------------ save
@pytest.mark.parametrize("n,m", SAVE_SHAPES)
def test_save(gpu, n, m):
    """a fresh solve keeps every problem's final working set, and every output stays the device entry's"""
    insts = save_instances(n, m)
    out, _, _ = fresh(insts)
    assert out.evicted == 0 and out.state.T.is_contiguous() and out.state.T.shape == (3, m, 1 + n + m)
    plain = sx.solve_batch_tensors(*tensors(insts), objective_row=True)
    assert plain.state is None
    same_tensors(out, plain)
    same_as_refs(out, [ref_with_row(*inst) for inst in insts], n, m)


def test_save_mixed_outcomes(gpu):
    """phase-1 states (INFEASIBLE) and phase-2 states (FEASIBLE, UNBOUNDED) side by side"""
    insts = mixed_instances()
    out, refs, _ = fresh(insts)
    assert {r["phase"] for r in refs} == {1, 2}
    assert {r["status"] for r in refs} == {sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED}
    same_tensors(out, sx.solve_batch_tensors(*tensors(insts), objective_row=True))


# ------------------------------------------------------------------ cap and resume
@pytest.mark.parametrize("n,m", CAP_SHAPES)
@pytest.mark.parametrize("cap", CAPS)
def test_cap_and_resume(gpu, n, m, cap):
    insts = cap_instances(n, m)
    cv = cap_value(cap, insts)
    whole = [ref_state(*inst) for inst in insts]
    capped, crefs, c = fresh(insts, cv)
    if cap in (1, 2):
        assert any(r["status"] == sx.PIVOT_CAP and r["phase"] == 1 for r in crefs)
    # a new state: the one-call solve in every output and in the state; the old state unchanged
    keep = clone(capped.state)
    done = sx.resume_batch_tensors(capped.state, c, objective_row=True, in_place=False)
    assert done.state is not capped.state and done.evicted == 0
    same_as_state_refs(done, whole, n, m)
    same_state(capped.state, keep)
    # a resume under the same cap changes nothing
    again = sx.resume_batch_tensors(capped.state, c, max_pivots=cv, objective_row=True, in_place=False)
    same_as_state_refs(again, crefs, n, m)
    # in place
    done2 = sx.resume_batch_tensors(capped.state, c, objective_row=True)
    assert done2.state is capped.state
    same_as_state_refs(done2, whole, n, m)
    same_tensors(done2, done)
    # a resume of a finished state changes nothing
    done3 = sx.resume_batch_tensors(done2.state, c, objective_row=True)
    same_as_state_refs(done3, whole, n, m)


# ------------------------------------------------------------------ ladder
@pytest.mark.parametrize("cap", LADDER_CAPS)
def test_ladder_capped_and_resumed(gpu, cap):
    """the continued selection walks the same eps-argmin tree: tie_ladders' B-small, whose pivots the
    lane tree decides in both phases, and its seed neighbours"""
    insts = ladder_instances()
    n, m = shape_of(insts)
    whole = [ref_state(*inst) for inst in insts]
    assert (whole[0]["status"], whole[0]["pivots"]) == (sx.FEASIBLE, tl.BATCH_CASES["B-small"][5])
    capped, _, c = fresh(insts, cap)
    done = sx.resume_batch_tensors(capped.state, c, objective_row=True)
    same_as_state_refs(done, whole, n, m)


# ------------------------------------------------------------------ structured LPs
@pytest.mark.parametrize("n,m", slp.SHAPES)
def test_structured_lps_capped_and_resumed(gpu, n, m):
    """the 22 instances of a shape capped at 3 pivots per phase, then resumed under the family's cap"""
    insts = structured_instances(n, m)
    whole = [ref_state(*inst, slp.cap(n, m)) for inst in insts]
    capped, _, c = fresh(insts, STRUCTURED_FIRST_CAP)
    done = sx.resume_batch_tensors(capped.state, c, max_pivots=slp.cap(n, m), objective_row=True)
    same_as_state_refs(done, whole, n, m)


# ------------------------------------------------------------------ evict and resume
def test_evict_and_resume(gpu):
    """a resident budget of 2 pivots per phase and call: an evicted problem is left with the state a
    cap of 2 leaves, and every resume takes it 2 pivots further in its phase"""
    insts = eviction_instances()
    n, m = shape_of(insts)
    whole = [ref_state(*inst) for inst in insts]
    cap2 = [ref_state(*inst, 2) for inst in insts]
    assert all(r["pivots"] == (2, 0) and r["phase"] == 1 for r in cap2)
    A, b, c = tensors(insts)
    bound = max(sum(r["pivots"]) for r in whole) // 2 + 2
    sx.set_batch_budget(2)
    try:
        out = sx.solve_batch_tensors(A, b, c, objective_row=True, keep_state=True)
        assert out.evicted == 4 and out.status.tolist() == [sx.NOT_ENDED] * 4
        assert out.pivots.tolist() == [[2, 0]] * 4
        # NOT_ENDED in the device entry's conventions, the state a cap of 2 leaves
        assert torch.isnan(out.optimal_value).all() and not out.solution.view(torch.int64).any()
        assert not out.objective_row.view(torch.int64).any() and not out.row_width.any()
        same_state(out.state, state_tensors(cap2))
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= bound, "an evicted problem does not progress"
            out = sx.resume_batch_tensors(out.state, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= max(r["pivots"][0] for r in whole) // 2 - 1
    same_as_state_refs(out, whole, n, m)


# ------------------------------------------------------------------ re-cost
@pytest.mark.parametrize("n,m", WARM_SHAPES)
def test_recost(gpu, n, m):
    """the warm start: phase 2 restarted on new costs from the saved optimum's tableau and basis"""
    insts = warm_instances(n, m)
    first, refs, _ = fresh(insts)
    keep = clone(first.state)
    for scale in WARM_SCALES:
        c2s = [warm_costs(inst[2], seed, scale) for inst, seed in zip(insts, WARM_SEEDS)]
        want = [ref_resume(r, c2, recost=True) for r, c2 in zip(refs, c2s)]
        c2 = torch.from_numpy(np.stack(c2s)).cuda()
        warm = sx.resume_batch_tensors(first.state, c2, objective_row=True, recost=True, in_place=False)
        same_as_state_refs(warm, want, n, m)
        assert all(w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
    same_state(first.state, keep)


def test_recost_mixed_phases(gpu):
    """one call over phase-1 states (capped or INFEASIBLE: continued, re-costing does not apply) and
    phase-2 states (re-costed with the next instance's costs), with c read through a strided view"""
    insts = mixed_instances()
    n, m = shape_of(insts)
    capped, refs, _ = fresh(insts, 15)
    assert sum(r["phase"] == 1 for r in refs) >= 10 and sum(r["phase"] == 2 for r in refs) >= 4
    assert any(r["phase"] == 1 and r["status"] == sx.PIVOT_CAP for r in refs)
    c2s = [insts[(k + 1) % len(insts)][2] for k in range(len(insts))]
    want = [ref_resume(r, c2, recost=True) for r, c2 in zip(refs, c2s)]
    assert len({w["status"] for w in want}) >= 3
    wide = torch.full((len(insts), 2 * n + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * n + 1:2] = torch.from_numpy(np.stack(c2s)).cuda()
    view = wide[:, 1:2 * n + 1:2]
    assert view.stride() == (2 * n + 3, 2)
    out = sx.resume_batch_tensors(capped.state, view, objective_row=True, recost=True)
    same_as_state_refs(out, want, n, m)


# ------------------------------------------------------------------ more problems than workgroups
def test_more_problems_than_resident_workgroups(gpu):
    """1,200 problems capped at 3 and resumed: a workgroup loads, solves and stores one state after another"""
    insts = many_instances()
    assert len(insts) == 1200
    whole = [ref_state(*inst) for inst in insts]
    capped, _, c = fresh(insts, MANY_CAP)
    done = sx.resume_batch_tensors(capped.state, c, objective_row=True)
    same_as_state_refs(done, whole, 5, 4)


# ------------------------------------------------------------------ bad states
@pytest.mark.parametrize("field,value,phase", [("phase", 0, 2), ("phase", 3, 1), ("base", -1, 2), ("base", "n+2m", 1),
                                               ("base", "n+m", 2), ("pivots", -1, 1), ("pivots0", -1, 1),
                                               ("pivots0", -1, 2)])
def test_bad_state(gpu, field, value, phase):
    """one problem of eight fails the kernel's checks: BAD_STATE and cleared outputs for it, the
    seven others exact.  n + m is a valid basis entry in phase 1 and is not one in phase 2"""
    n, m, bad = 20, 10, 5
    insts = bad_state_instances()
    start = [ref_state(*inst, BAD_STATE_PHASE1_CAP if phase == 1 else -1) for inst in insts]
    assert all(r["phase"] == phase for r in start)
    whole = [ref_state(*inst) for inst in insts]
    state = state_tensors(start)
    value = {"n+2m": n + 2 * m, "n+m": n + m}.get(value, value)
    if field == "phase":
        state.phase[bad] = value
    elif field == "base":
        state.base[bad, 3] = value
    else:  # either count alone
        state.pivots[bad, 0 if field == "pivots0" else 1] = value
    keep = clone(state)
    c = tensors(insts)[2]
    out = sx.resume_batch_tensors(state, c, objective_row=True, in_place=False)
    same_state(state, keep)
    assert out.evicted == 0
    assert int(out.status[bad]) == sx.BAD_STATE and out.pivots[bad].tolist() == [0, 0]
    assert torch.isnan(out.optimal_value[bad]) and not out.solution[bad].view(torch.int64).any()
    assert out.base[bad].tolist() == [-1] * m
    assert not out.objective_row[bad].view(torch.int64).any() and int(out.row_width[bad]) == 0
    assert int(out.state.phase[bad]) == 0
    # the others, as if the bad one were not there
    good = [k for k in range(8) if k != bad]
    pick = lambda t: t[good]  # noqa: E731
    rest = sx.BatchTensors(pick(out.status), pick(out.pivots), pick(out.optimal_value), pick(out.solution),
                           pick(out.base), pick(out.objective_row), pick(out.row_width), 0, None, None,
                           sx.BatchState(*(pick(getattr(out.state, f)) for f in STATE_FIELDS), n, m))
    same_as_state_refs(rest, [whole[k] for k in good], n, m)
    if phase == 1:  # the boundary on the other side: n + m is an artificial variable's index, valid in phase 1
        assert any((r["base"] >= n + m).any() for r in start)


# ------------------------------------------------------------------ stream
def test_non_default_stream(gpu):
    insts = mixed_instances()
    n, m = shape_of(insts)
    A, b, c = tensors(insts)
    crefs = [ref_state(*inst, 3) for inst in insts]
    whole = [ref_state(*inst) for inst in insts]
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.solve_batch_tensors(A, b, c, max_pivots=3, objective_row=True, finish=False, keep_state=True)
        done = sx.resume_batch_tensors(capped.state, c, objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, crefs, n, m)
    same_as_state_refs(done, whole, n, m)


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: a resume with A and b NULL, `out` NULL and every optional output NULL; a fresh
    solve with `out` NULL; a fresh solve whose state is kept while the optional outputs are NULL"""
    n, m = 20, 10
    insts = save_instances(n, m)
    B = len(insts)
    A, b, c = tensors(insts)
    crefs = [ref_state(*inst, 2) for inst in insts]
    whole = [ref_state(*inst) for inst in insts]
    state = state_tensors(crefs)
    keep = clone(state)

    o = state_call(n, m, B, dense(c), state_in=state, state_out=None, x=None, base=None, objrow=None, row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(state, keep)  # nothing was written to `in`
    assert o.status.tolist() == [r["status"] for r in whole]
    assert [tuple(p) for p in o.pivots.tolist()] == [r["pivots"] for r in whole]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([r["opt"] for r in whole]))
    assert int(o.evicted.item()) == 0

    # the same with outputs, into a new state
    new = sx.BatchState.empty(B, n, m, "cuda")
    o = state_call(n, m, B, dense(c), state_in=state, state_out=new)
    assert o.rc == 0
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, new)
    same_as_state_refs(got, whole, n, m)

    # fresh, nothing kept: the device entry
    o = state_call(n, m, B, dense(c), A=dense(A), b=dense(b))
    assert o.rc == 0
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()))
    same_as_refs(got, whole, n, m)

    # fresh, the state kept, the optional outputs NULL
    new = sx.BatchState.empty(B, n, m, "cuda")
    o = state_call(n, m, B, dense(c), A=dense(A), b=dense(b), state_out=new, max_pivots=2, x=None, base=None,
                   objrow=None, row_width=None)
    assert o.rc == 0 and o.status.tolist() == [sx.PIVOT_CAP] * B
    same_state(new, state)
    assert float(o.opt[0]) != SENTINEL
