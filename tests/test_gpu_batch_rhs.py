"""A kept batch state re-solved for a new right-hand side (simplex_solve_batch_device_rhs, sx_batch.hip
k_batch_solve_rhs) through sx.resume_batch_tensors(state, c, A=, b=), and through a ctypes caller
(device_entries.rhs_call) for what that never passes.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_rhs_refs.py: the entry
restated from the oracle's argmin, ratio, gemv_partials and apply_update (test_batch_rhs_host.py
shows on the CPU what the restatement reaches).  Compared per problem: status, both pivot counts, the
basis, objective and solution (NaN and zeros unless FEASIBLE), the objective row and its width, and
the saved T, d, base, phase and pivots."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_refs import same_tensors, tensors
from batch_rhs_refs import (CAP_SHAPE, PHASE2_CAP, PHASE2_CAP_SHAPE, RHS_CAPS, RHS_SCALES, RHS_SHAPES, first_min,
                            ladder_cases, negated_rhs, ref_rhs, ref_rhs_resume, rhs_instances, scaled_batch)
from batch_state_refs import (bits, many_instances, mixed_instances, ref_resume, ref_state, same_as_state_refs,
                              state_tensors)
from device_entries import dense, rhs_call

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")


def shape_of(insts):
    m, n = insts[0][0].shape
    return n, m


def kept(insts, max_pivots=-1):
    """one keep_state call, checked against the reference: (BatchTensors, refs, (A, b, c))"""
    A, b, c = tensors(insts)
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, *shape_of(insts))
    assert out.state.rhs is False
    return out, refs, (A, b, c)


def dev(rows):
    return torch.from_numpy(np.stack(rows)).cuda()


def rerhs(state, abc, b2s, **kw):
    kw.setdefault("in_place", False)
    out = sx.resume_batch_tensors(state, abc[2], objective_row=True, A=abc[0], b=dev(b2s), **kw)
    assert out.state.rhs is True
    return out


def want_rhs(refs, insts, b2s, max_pivots=-1):
    return [ref_rhs(r, A, b2, c, max_pivots) for r, (A, _, c), b2 in zip(refs, insts, b2s)]


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m, state.rhs)


def same_state(x, y):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in ("base", "phase", "pivots"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f


# ------------------------------------------------------------------ warm
@pytest.mark.parametrize("n,m", RHS_SHAPES)
def test_warm(gpu, n, m):
    """every b_i moved by up to 10 % and by up to 100 %: the dual loop from the kept optimum"""
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    keep = clone(first.state)
    for scale in RHS_SCALES:
        b2s = scaled_batch(insts, scale)
        want = want_rhs(refs, insts, b2s)
        if scale == 1.0 and (n, m) != (1, 1):
            assert any(w["dual"] >= 1 for w in want)
        assert all(w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
        out = rerhs(first.state, abc, b2s)
        assert out.evicted == 0
        same_as_state_refs(out, want, n, m)
    same_state(first.state, keep)


@pytest.mark.parametrize("n,m", RHS_SHAPES)
def test_negated_row_is_infeasible(gpu, n, m):
    """one b_i negated: INFEASIBLE inside the dual loop, kept as phase 3, and again without a pivot"""
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    b2s = [negated_rhs(inst[1], k + 1) for k, inst in enumerate(insts)]
    want = want_rhs(refs, insts, b2s)
    assert all(w["status"] == sx.INFEASIBLE and w["phase"] == 3 for w in want)
    out = rerhs(first.state, abc, b2s)
    same_as_state_refs(out, want, n, m)
    again = sx.resume_batch_tensors(out.state, abc[2], objective_row=True)
    assert again.state is out.state and again.state.rhs is True
    same_as_state_refs(again, want, n, m)


def test_mixed_states(gpu):
    """phase-1 states, UNBOUNDED phase-2 states and FEASIBLE ones in one call: the cold ones are
    solve_batch_tensors on the new right-hand side"""
    insts = mixed_instances()
    n, m = shape_of(insts)
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 0.1)
    want = want_rhs(refs, insts, b2s)
    cold = [k for k, w in enumerate(want) if "dual" not in w]
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold} == {(1, sx.INFEASIBLE), (2, sx.UNBOUNDED)}
    assert 0 < len(cold) < len(insts)
    out = rerhs(first.state, abc, b2s)
    same_as_state_refs(out, want, n, m)
    plain = sx.solve_batch_tensors(abc[0], dev(b2s), abc[2], objective_row=True)
    pick = lambda o: sx.BatchTensors(*(t[cold] for t in (o.status, o.pivots, o.optimal_value, o.solution, o.base,  # noqa: E731
                                                          o.objective_row, o.row_width)), 0)
    same_tensors(pick(out), pick(plain))


def test_state_capped_in_phase_2_is_a_cold_start(gpu):
    n, m = PHASE2_CAP_SHAPE
    insts = rhs_instances(n, m)
    capped, refs, abc = kept(insts, PHASE2_CAP)
    assert all(r["status"] == sx.PIVOT_CAP and r["phase"] == 2 for r in refs)
    b2s = scaled_batch(insts, 0.1)
    out = rerhs(capped.state, abc, b2s)
    same_as_state_refs(out, [ref_state(A, b2, c) for (A, _, c), b2 in zip(insts, b2s)], n, m)


# ------------------------------------------------------------------ cap, budget, re-entry
@pytest.mark.parametrize("cap", RHS_CAPS)
def test_cap_inside_the_dual_loop_and_resume(gpu, cap):
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    whole = want_rhs(refs, insts, b2s)
    crefs = want_rhs(refs, insts, b2s, cap)
    assert all(r["status"] == sx.PIVOT_CAP and r["phase"] == 3 and r["pivots"][1] == cap for r in crefs)
    capped = rerhs(first.state, abc, b2s, max_pivots=cap)
    same_as_state_refs(capped, crefs, n, m)
    # a new state: the uncapped call in every output and in the state; the old state unchanged
    keep = clone(capped.state)
    done = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True, in_place=False)
    assert done.state is not capped.state and done.state.rhs is True and done.evicted == 0
    same_as_state_refs(done, whole, n, m)
    same_state(capped.state, keep)
    # a resume under the same cap changes nothing
    again = sx.resume_batch_tensors(capped.state, abc[2], max_pivots=cap, objective_row=True, in_place=False)
    same_as_state_refs(again, crefs, n, m)
    # in place
    done2 = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True)
    assert done2.state is capped.state
    same_as_state_refs(done2, whole, n, m)
    same_tensors(done2, done)


def test_budget_inside_the_dual_loop(gpu):
    """a resident budget of 2 pivots per call: evicted inside the dual loop with the state a cap of 2
    leaves, and every plain resume takes it 2 pivots further"""
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    whole = want_rhs(refs, insts, b2s)
    cap2 = want_rhs(refs, insts, b2s, 2)
    bound = max(w["pivots"][1] for w in whole) // 2 + 2
    sx.set_batch_budget(2)
    try:
        out = rerhs(first.state, abc, b2s)
        assert out.evicted == 3 and out.status.tolist() == [sx.NOT_ENDED] * 3
        assert out.state.phase.tolist() == [3] * 3 and out.pivots[:, 1].tolist() == [2] * 3
        same_state(out.state, state_tensors(cap2))
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= bound, "an evicted problem does not progress"
            out = sx.resume_batch_tensors(out.state, abc[2], objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= min(w["dual"] for w in whole) // 2 - 1
    same_as_state_refs(out, whole, n, m)


def test_second_rerhs_on_a_phase_3_state(gpu):
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    crefs = want_rhs(refs, insts, b2s, 2)
    capped = rerhs(first.state, abc, b2s, max_pivots=2)
    assert capped.state.phase.tolist() == [3] * 3
    b3s = scaled_batch(insts, 0.1)
    want = want_rhs(crefs, insts, b3s)
    assert all("dual" in w and w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
    out = rerhs(capped.state, abc, b3s, in_place=True)
    assert out.state is capped.state
    same_as_state_refs(out, want, n, m)


# ------------------------------------------------------------------ the plain resume and the state entry
def test_plain_resume_of_phase_1_and_2_states_is_the_state_entry(gpu):
    insts = mixed_instances()
    n, m = shape_of(insts)
    capped, refs, abc = kept(insts, 15)
    assert {r["phase"] for r in refs} == {1, 2}
    through_state = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True, in_place=False)
    assert through_state.state.rhs is False
    mine = clone(capped.state)
    mine.rhs = True
    through_rhs = sx.resume_batch_tensors(mine, abc[2], objective_row=True, in_place=False)
    assert through_rhs.state.rhs is True
    same_tensors(through_rhs, through_state)
    same_state(through_rhs.state, through_state.state)
    same_as_state_refs(through_rhs, [ref_resume(r, inst[2]) for r, inst in zip(refs, insts)], n, m)


def test_phase_3_through_the_state_entry_is_a_bad_state(gpu):
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    capped = rerhs(first.state, abc, scaled_batch(insts, 1.0), max_pivots=2)
    assert capped.state.phase.tolist() == [3] * 3
    state = clone(capped.state)
    state.rhs = False  # what a caller of the C entries can do: hand a phase-3 state to the primal resume
    keep = clone(state)
    out = sx.resume_batch_tensors(state, abc[2], objective_row=True, in_place=False)
    same_state(state, keep)
    assert out.status.tolist() == [sx.BAD_STATE] * 3 and out.state.phase.tolist() == [0] * 3
    assert torch.isnan(out.optimal_value).all() and not out.solution.view(torch.int64).any()
    assert (out.base == -1).all() and not out.objective_row.view(torch.int64).any() and not out.row_width.any()
    # a re-cost is the state entry's too
    out = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True, recost=True, in_place=False)
    assert out.status.tolist() == [sx.BAD_STATE] * 3 and out.state.rhs is False


# ------------------------------------------------------------------ strides, many problems, a stream
def test_strided_b_and_transposed_a(gpu):
    n, m = 20, 10
    insts = rhs_instances(n, m)
    first, refs, (A, b, c) = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    want = want_rhs(refs, insts, b2s)
    wide = torch.full((len(insts), 2 * m + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * m + 1:2] = dev(b2s)
    view = wide[:, 1:2 * m + 1:2]
    assert view.stride() == (2 * m + 3, 2)
    At = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert At.stride() == (n * m, 1, m)
    out = sx.resume_batch_tensors(first.state, c, objective_row=True, in_place=False, A=At, b=view)
    same_as_state_refs(out, want, n, m)
    # the cold path reads b through its stride too
    cold = state_tensors([ref_state(*inst, 2) for inst in insts])
    out = sx.resume_batch_tensors(cold, c, objective_row=True, A=At, b=view)
    same_as_state_refs(out, [ref_state(A_, b2, c_) for (A_, _, c_), b2 in zip(insts, b2s)], n, m)


def test_more_problems_than_resident_workgroups(gpu):
    insts = many_instances()
    assert len(insts) == 1200
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    want = want_rhs(refs, insts, b2s)
    assert sum(w.get("dual", 0) >= 1 for w in want) >= 100
    out = rerhs(first.state, abc, b2s)
    same_as_state_refs(out, want, 5, 4)


def test_non_default_stream(gpu):
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    first, refs, abc = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    b2 = dev(b2s)
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.resume_batch_tensors(first.state, abc[2], max_pivots=2, objective_row=True, finish=False,
                                         in_place=False, A=abc[0], b=b2)
        done = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, want_rhs(refs, insts, b2s, 2), n, m)
    same_as_state_refs(done, want_rhs(refs, insts, b2s), n, m)


# ------------------------------------------------------------------ ladder
def test_ladder(gpu):
    """the leaving row of the dual loop is the eps-argmin tree's: on these right-hand sides the
    first exact minimum pivots another way (test_batch_rhs_host.py), the kernel the tree's"""
    cases = ladder_cases()
    insts = [inst for inst, _ in cases]
    n, m = shape_of(insts)
    first, refs, abc = kept(insts)
    b2s = [b2 for _, b2 in cases]
    want = want_rhs(refs, insts, b2s)
    for w, r, (A, _, c), b2 in zip(want, refs, insts, b2s):
        other = ref_rhs(r, A, b2, c, argmin=first_min)
        assert w["dual"] >= 1 and (w["pivots"] != other["pivots"] or not np.array_equal(w["base"], other["base"]))
    out = rerhs(first.state, abc, b2s)
    same_as_state_refs(out, want, n, m)


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: a re-rhs with `out` NULL and every optional output NULL; a plain resume of the
    phase-3 states with A and b NULL, into a new state"""
    n, m = CAP_SHAPE
    insts = rhs_instances(n, m)
    B = len(insts)
    first, refs, (A, b, c) = kept(insts)
    b2s = scaled_batch(insts, 1.0)
    b2 = dev(b2s)
    whole = want_rhs(refs, insts, b2s)
    keep = clone(first.state)

    o = rhs_call(n, m, B, dense(c), first.state, A=dense(A), b=dense(b2), rerhs=True, x=None, base=None, objrow=None,
                 row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(first.state, keep)  # nothing was written to `in`
    assert o.status.tolist() == [r["status"] for r in whole]
    assert [tuple(p) for p in o.pivots.tolist()] == [r["pivots"] for r in whole]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([r["opt"] for r in whole]))
    assert int(o.evicted.item()) == 0

    capped = sx.BatchState.empty(B, n, m, "cuda")
    o = rhs_call(n, m, B, dense(c), first.state, A=dense(A), b=dense(b2), state_out=capped, rerhs=True, max_pivots=2)
    assert o.rc == 0 and o.status.tolist() == [sx.PIVOT_CAP] * B
    new = sx.BatchState.empty(B, n, m, "cuda")
    o = rhs_call(n, m, B, dense(c), capped, state_out=new)
    assert o.rc == 0
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, new)
    same_as_state_refs(got, whole, n, m)
    same_as_state_refs(got, [ref_rhs_resume(r, inst[2]) for r, inst in zip(want_rhs(refs, insts, b2s, 2), insts)], n, m)
