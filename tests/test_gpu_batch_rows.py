"""A kept batch state grown by new constraint rows (simplex_solve_batch_device_rows, sx_batch.hip
k_batch_solve_rows) through sx.add_rows_batch_tensors, and through a ctypes caller (device_entries.rows_call) for
what that never passes.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_rows_refs.py: the entry
restated from batch_rhs_refs' dual loop, batch_state_refs._run and the oracle's fma
(test_batch_rows_host.py shows on the CPU what the restatement reaches).  Compared per problem:
status, both pivot counts, the basis, objective and solution (NaN and zeros unless FEASIBLE), the
objective row and its width, and the whole grown state: T, d, base, phase and pivots."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_refs import same_tensors, tensors
from batch_rhs_refs import ref_rhs, ref_rhs_resume, scaled_rhs
from batch_rows_refs import (CAP_SHAPE, KINDS, ROWS_CAPS, THETAS, cuts_off, grow, make_row, ref_rows, rows_instances,
                             rows_shapes, want_batch)
from batch_state_refs import (bits, many_instances, mixed_instances, ref_state, same_as_state_refs, state_tensors)
from device_entries import dense, rows_call

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")


def kept(insts, max_pivots=-1):
    """one keep_state call, checked against the reference: (BatchTensors, refs)"""
    A, b, c = tensors(insts)
    m, n = insts[0][0].shape
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, n, m)
    return out, refs


def add(state, grown, **kw):
    """the rows of `grown` (instances in the grown shape) added to `state`"""
    A, b, c = tensors(grown)
    out = sx.add_rows_batch_tensors(state, A, b, c, objective_row=True, **kw)
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
@pytest.mark.parametrize("n,m0,q", rows_shapes())
def test_shapes(gpu, n, m0, q):
    """a cut that excludes the kept optimum (the dual loop pivots), one that does not (no pivot), and
    a branch up that excludes it, on every shape: the in-state's dense stride 1 + n + m0 in both
    parities, q = 3, the LDS class, the workspace class and the step from one to the other, the new
    row first in a second row tile, the entering ratio over two tiles"""
    first, refs = kept(rows_instances(n, m0))
    keep = clone(first.state)
    for kind, theta in (("cut", 0.5), ("cut", 1.5), ("up", 1.5)):
        _, grown, _, want = want_batch(n, m0, q, kind, theta)
        assert all("dual" in w for w in want)
        if n > 1 or kind == "cut":
            assert any(w["dual"] >= 1 for w in want) == cuts_off(kind, theta)
        assert all(w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
        out = add(first.state, grown)
        assert out.evicted == 0
        same_as_state_refs(out, want, n, m0 + q)
    same_state(first.state, keep)


# ------------------------------------------------------------------ cold and warm in one batch
def test_mixed_states(gpu):
    """phase-1 (INFEASIBLE), UNBOUNDED and FEASIBLE states in one call: the cold ones are
    solve_batch_tensors on the grown problem"""
    insts = mixed_instances()
    m0, n = insts[0][0].shape
    first, refs = kept(insts)
    grown = [(np.vstack([A, np.ones(n)]), np.append(b, 50.0), c) for A, b, c in insts]
    want = [ref_rows(r, *g) for r, g in zip(refs, grown)]
    cold = [k for k, w in enumerate(want) if "dual" not in w]
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold} == {(1, sx.INFEASIBLE), (2, sx.UNBOUNDED)}
    assert 0 < len(cold) < len(insts)
    out = add(first.state, grown)
    same_as_state_refs(out, want, n, m0 + 1)
    plain = sx.solve_batch_tensors(*tensors(grown), objective_row=True)
    pick = lambda o: sx.BatchTensors(*(t[cold] for t in (o.status, o.pivots, o.optimal_value, o.solution, o.base,  # noqa: E731
                                                          o.objective_row, o.row_width)), 0)
    same_tensors(pick(out), pick(plain))


# ------------------------------------------------------------------ every kind of row
@pytest.mark.parametrize("n,m0", [(20, 10), (33, 31)])
def test_every_kind_of_row(gpu, n, m0):
    """cut, branch down and branch up at both thetas, and the impossible row, which ends INFEASIBLE
    inside the dual loop (phase 3) and again, without a pivot, when that state is re-entered"""
    first, _ = kept(rows_instances(n, m0))
    for kind in KINDS:
        for theta in THETAS:
            _, grown, _, want = want_batch(n, m0, 1, kind, theta)
            same_as_state_refs(add(first.state, grown), want, n, m0 + 1)
    _, grown, _, want = want_batch(n, m0, 1, "never", 0.5)
    assert all(w["status"] == sx.INFEASIBLE and w["phase"] == 3 for w in want)
    out = add(first.state, grown)
    same_as_state_refs(out, want, n, m0 + 1)
    again = sx.resume_batch_tensors(out.state, tensors(grown)[2], objective_row=True)
    assert again.state is out.state and again.state.rhs is True
    same_as_state_refs(again, want, n, m0 + 1)


def test_three_kinds_in_one_call(gpu):
    """q = 3 with a cut, a branch down and a branch up side by side"""
    n, m0 = 5, 4
    insts = rows_instances(n, m0)
    first, refs = kept(insts)
    for theta in THETAS:
        grown = [grow(inst, KINDS, theta) for inst in insts]
        want = [ref_rows(r, *g) for r, g in zip(refs, grown)]
        assert any(w["dual"] >= 1 for w in want)
        same_as_state_refs(add(first.state, grown), want, n, m0 + 3)


# ------------------------------------------------------------------ cap, budget
@pytest.mark.parametrize("cap", ROWS_CAPS)
def test_cap_inside_the_dual_loop_and_resume(gpu, cap):
    n, m0, q = CAP_SHAPE
    insts, grown, refs, whole = want_batch(n, m0, q, "cut", 0.5)
    crefs = want_batch(n, m0, q, "cut", 0.5, cap)[3]
    assert all(r["status"] == sx.PIVOT_CAP and r["phase"] == 3 and r["pivots"][1] == cap for r in crefs)
    first, _ = kept(insts)
    capped = add(first.state, grown, max_pivots=cap)
    same_as_state_refs(capped, crefs, n, m0 + q)
    c = tensors(grown)[2]
    keep = clone(capped.state)
    done = sx.resume_batch_tensors(capped.state, c, objective_row=True, in_place=False)
    assert done.state.rhs is True and done.evicted == 0
    same_as_state_refs(done, whole, n, m0 + q)
    same_state(capped.state, keep)
    again = sx.resume_batch_tensors(capped.state, c, max_pivots=cap, objective_row=True, in_place=False)
    same_as_state_refs(again, crefs, n, m0 + q)


def test_budget_inside_the_dual_loop(gpu):
    """a resident budget of 2 pivots per call: evicted inside the dual loop with the state a cap of 2
    leaves, and every plain resume takes it 2 pivots further, until nothing is evicted"""
    n, m0, q = CAP_SHAPE
    insts, grown, refs, whole = want_batch(n, m0, q, "cut", 0.5)
    cap2 = want_batch(n, m0, q, "cut", 0.5, 2)[3]
    first, _ = kept(insts)
    c = tensors(grown)[2]
    bound = max(w["pivots"][1] for w in whole) // 2 + 2
    sx.set_batch_budget(2)
    try:
        out = add(first.state, grown)
        assert out.evicted == 3 and out.status.tolist() == [sx.NOT_ENDED] * 3
        assert out.state.phase.tolist() == [3] * 3 and out.pivots[:, 1].tolist() == [2] * 3
        same_state(out.state, state_tensors(cap2))
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= bound, "an evicted problem does not progress"
            out = sx.resume_batch_tensors(out.state, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= min(w["dual"] for w in whole) // 2 - 1
    same_as_state_refs(out, whole, n, m0 + q)


# ------------------------------------------------------------------ chains
def test_row_then_new_rhs_then_row(gpu):
    """the grown state is a state of the right-hand-side entry: a new b [m] on it, then another row"""
    n, m0 = 20, 10
    insts, grown, refs, want = want_batch(n, m0, 1, "cut", 0.5)
    first, _ = kept(insts)
    one = add(first.state, grown)
    same_as_state_refs(one, want, n, m0 + 1)
    A, b, c = tensors(grown)
    b2s = [scaled_rhs(g[1], 1000 + k, 0.3) for k, g in enumerate(grown)]
    want2 = [ref_rhs(w, g[0], b2, g[2]) for w, g, b2 in zip(want, grown, b2s)]
    two = sx.resume_batch_tensors(one.state, c, objective_row=True, in_place=False, A=A, b=dev(b2s))
    same_as_state_refs(two, want2, n, m0 + 1)
    assert all(w["status"] == sx.FEASIBLE for w in want2) and any(w["dual"] >= 1 for w in want2)
    grown3 = [grow((g[0], b2, g[2]), ["down"], 0.5) for g, b2 in zip(grown, b2s)]
    want3 = [ref_rows(w, *g) for w, g in zip(want2, grown3)]
    assert any(w["dual"] >= 1 for w in want3)
    three = add(two.state, grown3)
    same_as_state_refs(three, want3, n, m0 + 2)


def test_row_on_a_phase_3_state(gpu):
    """a row added to states that a capped re-rhs left inside the dual loop"""
    n, m0 = 64, 63
    insts = rows_instances(n, m0)
    first, refs = kept(insts)
    A, b, c = tensors(insts)
    b2s = [inst[1] * (1.0 + np.random.default_rng(k).uniform(-1.0, 1.0, size=m0)) for k, inst in enumerate(insts)]
    crefs = [ref_rhs(r, inst[0], b2, inst[2], 2) for r, inst, b2 in zip(refs, insts, b2s)]
    assert [r["phase"] for r in crefs] == [3] * 3
    capped = sx.resume_batch_tensors(first.state, c, max_pivots=2, objective_row=True, in_place=False, A=A, b=dev(b2s))
    same_as_state_refs(capped, crefs, n, m0)
    rows = [make_row(inst, "cut", 0.5) for inst in insts]
    grown = [(np.vstack([inst[0], a]), np.append(b2, beta), inst[2]) for inst, b2, (a, beta) in zip(insts, b2s, rows)]
    want = [ref_rows(r, *g) for r, g in zip(crefs, grown)]
    assert all("dual" in w and w["pivots"][0] == r["pivots"][0] for w, r in zip(want, refs))
    same_as_state_refs(add(capped.state, grown), want, n, m0 + 1)


# ------------------------------------------------------------------ strides, many problems, a stream
def test_strided_b_and_transposed_a(gpu):
    n, m0 = 20, 10
    m = m0 + 1
    insts, grown, refs, want = want_batch(n, m0, 1, "cut", 0.5)
    first, _ = kept(insts)
    A, b, c = tensors(grown)
    wide = torch.full((len(insts), 2 * m + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * m + 1:2] = b
    view = wide[:, 1:2 * m + 1:2]
    assert view.stride() == (2 * m + 3, 2)
    At = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert At.stride() == (n * m, 1, m)
    out = sx.add_rows_batch_tensors(first.state, At, view, c, objective_row=True)
    same_as_state_refs(out, want, n, m)
    # the cold path reads A and b through their strides too
    cold = state_tensors([ref_state(*inst, 2) for inst in insts])
    assert cold.phase.tolist() == [1] * 3
    out = sx.add_rows_batch_tensors(cold, At, view, c, objective_row=True)
    same_as_state_refs(out, [ref_state(*g) for g in grown], n, m)


def test_more_problems_than_resident_workgroups(gpu):
    insts = many_instances()
    assert len(insts) == 1200
    first, refs = kept(insts)
    grown = [grow(inst, ["cut"], 0.5) for inst in insts]
    want = [ref_rows(r, *g) for r, g in zip(refs, grown)]
    assert sum(w["dual"] >= 1 for w in want) >= 100
    same_as_state_refs(add(first.state, grown), want, 5, 5)


def test_non_default_stream(gpu):
    n, m0, q = CAP_SHAPE
    insts, grown, refs, whole = want_batch(n, m0, q, "cut", 0.5)
    first, _ = kept(insts)
    A, b, c = tensors(grown)
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.add_rows_batch_tensors(first.state, A, b, c, max_pivots=2, objective_row=True, finish=False)
        done = sx.resume_batch_tensors(capped.state, c, objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, want_batch(n, m0, q, "cut", 0.5, 2)[3], n, m0 + q)
    same_as_state_refs(done, whole, n, m0 + q)


# ------------------------------------------------------------------ bad states
def test_bad_states(gpu):
    """a base entry that the grown shape would accept but the in-state's does not, phase 0 and a
    negative pivot count: BAD_STATE, cleared outputs and phase 0 for that problem alone"""
    n, m0 = 20, 10
    insts = rows_instances(n, m0) + rows_instances(n, m0)[:1]
    grown = [grow(inst, ["cut"], 0.5) for inst in insts]
    first, refs = kept(insts)
    state = clone(first.state)
    state.base[0, 3] = n + m0       # < n + m0 + 1: the new row's own slack, not a variable of the in-state
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
    from batch_refs import same_as_refs
    same_as_refs(good, [ref_rows(refs[3], *grown[3])], n, m0 + 1)


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: `out` NULL and every optional output NULL; then into a state with the outputs"""
    n, m0, q = CAP_SHAPE
    m = m0 + q
    insts, grown, refs, whole = want_batch(n, m0, q, "cut", 0.5)
    B = len(insts)
    first, _ = kept(insts)
    A, b, c = tensors(grown)
    keep = clone(first.state)
    o = rows_call(n, m, B, dense(A), dense(b), dense(c), first.state, q, x=None, base=None, objrow=None, row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(first.state, keep)  # nothing was written to `in`
    assert o.status.tolist() == [r["status"] for r in whole]
    assert [tuple(p) for p in o.pivots.tolist()] == [r["pivots"] for r in whole]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([r["opt"] for r in whole]))
    assert int(o.evicted.item()) == 0
    capped = sx.BatchState.empty(B, n, m, "cuda")
    o = rows_call(n, m, B, dense(A), dense(b), dense(c), first.state, q, state_out=capped, max_pivots=2)
    assert o.rc == 0 and o.status.tolist() == [sx.PIVOT_CAP] * B
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, capped)
    crefs = want_batch(n, m0, q, "cut", 0.5, 2)[3]
    same_as_state_refs(got, crefs, n, m)
    capped.rhs = True
    done = sx.resume_batch_tensors(capped, c, objective_row=True)
    same_as_state_refs(done, [ref_rhs_resume(r, g[2]) for r, g in zip(crefs, grown)], n, m)
    same_as_state_refs(done, whole, n, m)
