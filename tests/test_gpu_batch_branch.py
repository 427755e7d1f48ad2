"""Branching a kept batch state (simplex_solve_batch_device_branch, sx_batch.hip k_batch_solve_branch)
through sx.branch_batch_tensors, and through a ctypes caller (device_entries.branch_call) for what that
never passes.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_branch_refs.py: the existing
restatement of the rows entry (batch_rows_refs.ref_rows) on the explicit child
(test_batch_branch_host.py shows on the CPU what that reaches).  Compared per child: status, both pivot
counts, the basis, objective and solution (NaN and zeros unless FEASIBLE), the objective row and its
width, and the whole out-state: T, d, base, phase and pivots."""
import itertools

import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_branch_refs import (EDGE_SHAPES, LEVEL1, LEVEL2, PARENTS, THETAS, bound, branch_shapes, explicit, is_cold,
                               many_parents, mixed_levels, ref_branch, two_children, want_children,
                               want_two_children)
from batch_refs import same_tensors, tensors
from batch_rows_refs import CAP_SHAPE, ROWS_CAPS, optimum, rows_instances
from batch_state_refs import bits, ref_state, same_as_state_refs, state_tensors
from device_entries import Src, branch_call, dense, flipped, unchanged

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")
OUTPUTS = ("status", "pivots", "optimal_value", "solution", "base", "objective_row", "row_width")


def kept(insts, max_pivots=-1):
    """one keep_state call, checked against the reference: (BatchTensors, refs)"""
    A, b, c = tensors(insts)
    m, n = insts[0][0].shape
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, n, m)
    return out, refs


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def branch(state, roots, parent, tri, root=None, **kw):
    """the children of `state` on the root instances `roots`; tri = (var, coef, rhs) as arrays [C, q]"""
    A, b, c = tensors(roots)
    var, coef, rhs = tri
    kw.setdefault("objective_row", True)
    out = sx.branch_batch_tensors(state, i32(parent), i32(var), f64(coef), f64(rhs), A, b, c,
                                  root=None if root is None else i32(root), **kw)
    m = roots[0][0].shape[0] + np.asarray(var).shape[1]
    if kw.get("keep_state", True):
        assert out.state is not state and out.state.rhs is True and (out.state.n, out.state.m) == (state.n, m)
        assert out.state.phase.shape[0] == len(parent)
    else:
        assert out.state is None
    return out


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m, state.rhs)


def gather(state, idx):
    """the state's problems idx, copied: what a caller without the branch entry has to make"""
    at = torch.as_tensor(idx, dtype=torch.int64, device="cuda")
    return sx.BatchState(*(getattr(state, f).index_select(0, at) for f in STATE_FIELDS), state.n, state.m, state.rhs)


def same_state(x, y):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in ("base", "phase", "pivots"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f


def pick(out, keep):
    """the children `keep` of a BatchTensors, without the state"""
    return sx.BatchTensors(*(getattr(out, f)[keep] for f in OUTPUTS), 0)


def tile(row, C):
    """one list of bound rows [(var, coef, rhs)] for every child: (var [C, q], coef, rhs)"""
    var, coef, rhs = zip(*row)
    return (np.tile(np.array(var, dtype=np.int32), (C, 1)), np.tile(np.array(coef), (C, 1)),
            np.tile(np.array(rhs), (C, 1)))


# ------------------------------------------------------------------ two children per parent, each shape
@pytest.mark.parametrize("n,m0", branch_shapes())
def test_two_children_per_parent(gpu, n, m0):
    """down and up through the kept optimum's largest component at theta 0.5 and 1.5 -- in every call
    some children pivot in the dual loop and some do not -- with the parents in order and with a
    repeated, permuted list that leaves parent 1 out, on every shape: the in-state's dense stride in
    both parities, the 64-row class edge, LDS to workspace, workspace to workspace, the new row first in
    a second row tile, the entering ratio over two tiles.  At the edge shapes also against
    add_rows_batch_tensors on gathered copies of the state and the explicit A.  The in-state is left
    as it was"""
    insts = rows_instances(n, m0)
    first, refs = kept(insts)
    keep = clone(first.state)
    for theta in THETAS:
        for parent in PARENTS:
            _, _, tri, want = want_two_children(n, m0, parent, theta)
            assert not any(is_cold(w) for w in want)
            assert any(w["dual"] == 0 for w in want) and (n == 1 or any(w["dual"] >= 1 for w in want))
            out = branch(first.state, insts, parent, tri)
            assert out.evicted == 0
            same_as_state_refs(out, want, n, m0 + 1)
            if (n, m0) in EDGE_SHAPES:
                grown = [explicit(insts[p], tri[0][k], tri[1][k], tri[2][k]) for k, p in enumerate(parent)]
                rows = sx.add_rows_batch_tensors(gather(first.state, parent), *tensors(grown), objective_row=True)
                same_tensors(out, rows)
                same_state(out.state, rows.state)
    same_state(first.state, keep)


# ------------------------------------------------------------------ cold and warm in one call, and depth
def test_cold_and_warm_children_and_a_second_level(gpu):
    """the 24 mixed instances: level 1 (q = 1) has cold children from phase-1 and UNBOUNDED parents and
    warm ones; at level 2 (q = 2, on level 1's out-state) most go cold again, so the composite build sees
    two bound rows, one of them negated, and 8, 14 and 21 are warm behind a cold level 1.  The cold
    children are solve_batch_tensors on the explicit child"""
    insts, refs, one, two = mixed_levels()
    C, (m0, n) = len(insts), insts[0][0].shape
    cold1 = [k for k, w in enumerate(one) if is_cold(w)]
    cold2 = [k for k, w in enumerate(two) if is_cold(w)]
    assert 0 < len(cold1) < C and 0 < len(cold2) < C
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold1} == {(1, sx.INFEASIBLE), (2, sx.UNBOUNDED)}
    assert {8, 14, 21} <= set(cold1) - set(cold2) and not {9, 19, 23} & (set(cold1) | set(cold2))
    first, _ = kept(insts)
    parent = list(range(C))
    state = first.state
    for q, rows, want, cold in ((1, [LEVEL1], one, cold1), (2, [LEVEL1, LEVEL2], two, cold2)):
        tri = tile(rows, C)
        out = branch(state, insts, parent, tri)
        same_as_state_refs(out, want, n, m0 + q)
        grown = [explicit(inst, *zip(*rows)) for inst in insts]
        plain = sx.solve_batch_tensors(*tensors(grown), objective_row=True)
        same_tensors(pick(out, cold), pick(plain, cold))
        state = out.state


def test_third_level_general_coefficient_and_negative_zero(gpu):
    """q = 3 on the (5, 4) instances: behind a branch down and a branch up, two children per parent with
    2.5 x_j <= 0.625 x*_j and 2.5 x_i <= -0.0; warm from level 2's out-state, and cold -- the composite
    build over three bound rows, one negated, one with the right-hand side -0.0 -- from phase-1 states
    of the level-2 problems"""
    n, m0 = 5, 4
    insts = rows_instances(n, m0)
    first, refs = kept(insts)
    js = [int(np.argmax(optimum(inst))) for inst in insts]
    lvl = [[bound(inst, "down", 0.5), ((j + 1) % n, -1.0, -0.01)] for inst, j in zip(insts, js)]
    parent = [0, 1, 2]
    cut = lambda t: tuple(np.array([[r[f] for r in rows[:t]] for rows in lvl]) for f in range(3))  # noqa: E731
    one = branch(first.state, insts, parent, cut(1))
    want1 = want_children(refs, insts, parent, parent, *cut(1))
    same_as_state_refs(one, want1, n, m0 + 1)
    two = branch(one.state, insts, parent, cut(2))
    want2 = want_children(want1, insts, parent, parent, *cut(2))
    same_as_state_refs(two, want2, n, m0 + 2)
    parent3 = [0, 0, 1, 1, 2, 2]
    rows3 = []
    for k, p in enumerate(parent3):
        x = optimum(insts[p])
        last = (js[p], 2.5, 2.5 * 0.25 * x[js[p]]) if k % 2 == 0 else ((js[p] + 2) % n, 2.5, -0.0)
        rows3.append(lvl[p] + [last])
    tri3 = tuple(np.array([[r[f] for r in rows] for rows in rows3]) for f in range(3))
    assert np.signbit(tri3[2][1, 2]) and tri3[2][1, 2] == 0.0
    want3 = want_children(want2, insts, parent3, parent3, *tri3)
    assert not any(is_cold(w) for w in want3) and any(w["dual"] >= 1 for w in want3)
    three = branch(two.state, insts, parent3, tri3)
    same_as_state_refs(three, want3, n, m0 + 3)
    # the same children from phase-1 parents: cold, all three bound rows built from the triples
    capped = [ref_state(*explicit(inst, *zip(*rows)), 1) for inst, rows in zip(insts, lvl)]
    assert [s["phase"] for s in capped] == [1] * 3
    cold3 = want_children(capped, insts, parent3, parent3, *tri3)
    assert all(is_cold(w) for w in cold3)
    out = branch(state_tensors(capped), insts, parent3, tri3)
    same_as_state_refs(out, cold3, n, m0 + 3)
    grown = [explicit(insts[p], *zip(*rows)) for p, rows in zip(parent3, rows3)]
    same_tensors(pick(out, slice(None)), pick(sx.solve_batch_tensors(*tensors(grown), objective_row=True), slice(None)))


# ------------------------------------------------------------------ roots apart from parents
def test_roots_apart_from_parents(gpu):
    """R = 2 roots: level 1 with root=None (the parents are the roots), then P = 4 parents of those two
    roots with an explicit root list, in order and permuted"""
    n, m0 = 20, 10
    roots = rows_instances(n, m0)[:2]
    first, refs = kept(roots)
    p1 = [0, 0, 1, 1]
    tri1 = two_children(roots, p1, 0.5)
    want1 = want_children(refs, roots, p1, p1, *tri1)
    one = branch(first.state, roots, p1, tri1)
    same_as_state_refs(one, want1, n, m0 + 1)
    for p2 in ([0, 0, 1, 1, 2, 2, 3, 3], [3, 1, 0, 2, 2, 0, 1, 3]):
        root = [p // 2 for p in p2]
        new = [((int(tri1[0][p, 0]) + 1 + k % 3) % n,) + ((1.0, 3.0) if k % 2 == 0 else (-1.0, -0.25))
               for k, p in enumerate(p2)]
        tri2 = tuple(np.array([[tri1[f][p, 0], row[f]] for p, row in zip(p2, new)]) for f in range(3))
        want2 = want_children(want1, roots, p2, root, *tri2)
        assert any(w["dual"] >= 1 for w in want2)
        two = branch(one.state, roots, p2, tri2, root=root)
        same_as_state_refs(two, want2, n, m0 + 2)
    with pytest.raises(ValueError, match="without root the parents are the roots"):
        branch(one.state, roots, p2, tri2)


# ------------------------------------------------------------------ cap, strong branching, budget
@pytest.mark.parametrize("cap", ROWS_CAPS)
def test_cap_inside_the_dual_loop_resume_and_strong_branching(gpu, cap):
    n, m0, _ = CAP_SHAPE
    insts = rows_instances(n, m0)
    first, _ = kept(insts)
    parent = PARENTS[0]
    c = tensors(insts)[2][torch.as_tensor(parent, device="cuda")]
    stopped = 0
    for theta in THETAS:
        _, _, tri, whole = want_two_children(n, m0, parent, theta)
        crefs = want_two_children(n, m0, parent, theta, cap)[3]
        inside = [k for k, w in enumerate(whole) if w["dual"] > cap]
        stopped += len(inside)
        assert all((crefs[k]["status"], crefs[k]["phase"], crefs[k]["pivots"][1]) == (sx.PIVOT_CAP, 3, cap)
                   for k in inside)
        capped = branch(first.state, insts, parent, tri, max_pivots=cap)
        same_as_state_refs(capped, crefs, n, m0 + 1)
        keep = clone(capped.state)
        done = sx.resume_batch_tensors(capped.state, c, objective_row=True, in_place=False)
        assert done.state.rhs is True and done.evicted == 0
        same_as_state_refs(done, whole, n, m0 + 1)
        same_state(capped.state, keep)
        # strong branching: no state kept, the same outputs, the dual bound in objective_row[:, 0]
        probe = branch(first.state, insts, parent, tri, max_pivots=cap, keep_state=False)
        same_tensors(probe, capped)
        assert np.array_equal(bits(probe.objective_row[:, 0].cpu().numpy()), bits([r["d"][0] for r in crefs]))
        assert torch.isnan(probe.optimal_value[inside]).all()
    assert stopped >= 1


def test_budget_of_one_pivot(gpu):
    """a resident budget of one pivot per call: children that need more are evicted inside the dual loop
    with the state a cap of 1 leaves, and every plain resume takes them a pivot further"""
    n, m0, _ = CAP_SHAPE
    insts = rows_instances(n, m0)
    first, _ = kept(insts)
    parent = PARENTS[0]
    _, _, tri, whole = want_two_children(n, m0, parent, 0.5)
    cap1 = want_two_children(n, m0, parent, 0.5, 1)[3]
    c = tensors(insts)[2][torch.as_tensor(parent, device="cuda")]
    inside = [k for k, w in enumerate(whole) if w["dual"] >= 2]
    assert len(inside) == 3
    bound_calls = max(w["pivots"][1] for w in whole) + 2
    sx.set_batch_budget(1)
    try:
        out = branch(first.state, insts, parent, tri)
        assert out.evicted == (out.status == sx.NOT_ENDED).sum().item() >= len(inside)
        assert out.status[inside].tolist() == [sx.NOT_ENDED] * 3
        assert out.state.phase[inside].tolist() == [3] * 3 and out.pivots[inside, 1].tolist() == [1] * 3
        same_state(gather(out.state, inside), gather(state_tensors(cap1), inside))
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= bound_calls, "an evicted child does not progress"
            out = sx.resume_batch_tensors(out.state, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= min(whole[k]["dual"] for k in inside) - 1
    same_as_state_refs(out, whole, n, m0 + 1)


# ------------------------------------------------------------------ strides, a stream, many children
def test_strided_b_and_transposed_a(gpu):
    n, m0 = 20, 10
    parent = PARENTS[1]
    insts, refs, tri, want = want_two_children(n, m0, parent, 0.5)
    first, _ = kept(insts)
    A, b, c = tensors(insts)
    wide = torch.full((len(insts), 2 * m0 + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * m0 + 1:2] = b
    view = wide[:, 1:2 * m0 + 1:2]
    assert view.stride() == (2 * m0 + 3, 2)
    At = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert At.stride() == (n * m0, 1, m0)
    lists = (i32(parent), i32(tri[0]), f64(tri[1]), f64(tri[2]))
    out = sx.branch_batch_tensors(first.state, *lists, At, view, c, objective_row=True)
    same_as_state_refs(out, want, n, m0 + 1)
    # the cold path reads the roots through their strides too; the lists may be views
    cold = [ref_state(*inst, 2) for inst in insts]
    assert [s["phase"] for s in cold] == [1] * 3
    wide_lists = [torch.stack([t, t], dim=-1)[..., 0] for t in lists]
    assert not any(t.is_contiguous() for t in wide_lists[1:])
    out = sx.branch_batch_tensors(state_tensors(cold), *wide_lists, At, view, c, objective_row=True)
    same_as_state_refs(out, want_children(cold, insts, parent, parent, *tri), n, m0 + 1)


def test_non_default_stream(gpu):
    n, m0, _ = CAP_SHAPE
    parent = PARENTS[0]
    insts, refs, tri, whole = want_two_children(n, m0, parent, 0.5)
    first, _ = kept(insts)
    A, b, c = tensors(insts)
    lists = (i32(parent), i32(tri[0]), f64(tri[1]), f64(tri[2]))
    cc = c[torch.as_tensor(parent, device="cuda")]
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.branch_batch_tensors(first.state, *lists, A, b, c, max_pivots=2, objective_row=True, finish=False)
        done = sx.resume_batch_tensors(capped.state, cc, objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, want_two_children(n, m0, parent, 0.5, 2)[3], n, m0 + 1)
    same_as_state_refs(done, whole, n, m0 + 1)


def test_more_children_than_resident_workgroups(gpu):
    insts, parent = many_parents()
    assert len(insts) == 1200 and len(parent) == 2400
    first, refs = kept(insts)
    tri = two_children(insts, parent, 0.5)
    want = want_children(refs, insts, parent, parent, *tri)
    assert sum(w["dual"] >= 1 for w in want) >= 100
    same_as_state_refs(branch(first.state, insts, parent, tri), want, 5, 5)


def test_one_root_with_batch_strides_of_zero(gpu):
    """R = 1 through the C entry: A_sb = b_sb = c_sb = 0; P = 2 states of that root, one of them in
    phase 1, so both the warm and the cold path read the root through those strides"""
    n, m0 = 20, 10
    inst = rows_instances(n, m0)[0]
    states = [ref_state(*inst), ref_state(*inst, 2)]
    assert [s["phase"] for s in states] == [2, 1]
    parent = [0, 0, 1, 1]
    tri = two_children([inst, inst], parent, 0.5)
    want = want_children(states, [inst], parent, [0] * 4, *tri)
    assert [is_cold(w) for w in want] == [False, False, True, True]
    A, b, c = (t[0] for t in tensors([inst]))
    out = sx.BatchState.empty(4, n, m0 + 1, "cuda")
    o = branch_call(n, m0 + 1, 4, Src(A.data_ptr(), (0, n, 1), A), Src(b.data_ptr(), (0, 1), b),
                    Src(c.data_ptr(), (0, 1), c), state_tensors(states), 1, i32(parent), i32(tri[0]), f64(tri[1]),
                    f64(tri[2]), root=i32([0] * 4), state_out=out)
    assert o.rc == 0
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, out)
    same_as_state_refs(got, want, n, m0 + 1)


# ------------------------------------------------------------------ bad indices and states
def test_bad_indices_and_states(gpu):
    """one child each with parent = -1, parent = P, root = R, var = n, var = -1 and a parent whose phase
    is 7, among six good children: BAD_STATE, cleared outputs and out-phase 0 for those alone, the
    others bit for bit; the guarded sources and the in-state are left as they were"""
    n, m0 = 20, 10
    insts = rows_instances(n, m0)
    first, refs = kept(insts)
    state = gather(first.state, [0, 1, 2, 0])
    state.phase[3] = 7
    P, R = 4, 3
    keep = clone(state)
    good_parent = PARENTS[1]
    var, coef, rhs = (np.concatenate([t, t]) for t in want_two_children(n, m0, good_parent, 0.5)[2])
    want = want_two_children(n, m0, good_parent, 0.5)[3]
    parent = good_parent + [-1, P, 2, 0, 0, 3]
    root = good_parent + [2, 0, R, 0, 0, 0]
    var[9, 0], var[10, 0] = n, -1
    bad = list(range(6, 12))
    A, b, c = (np.stack([inst[f] for inst in insts]) for f in range(3))
    srcs = [flipped(a) for a in (A, b, c)]
    out = sx.BatchState.empty(12, n, m0 + 1, "cuda")
    o = branch_call(n, m0 + 1, 12, *srcs, state, R, i32(parent), i32(var), f64(coef), f64(rhs), root=i32(root),
                    state_out=out)
    assert o.rc == 0 and int(o.evicted.item()) == 0
    assert o.status.tolist() == [w["status"] for w in want] + [sx.BAD_STATE] * 6
    assert out.phase[bad].tolist() == [0] * 6 and not o.pivots[bad].any()
    assert torch.isnan(o.opt[bad]).all() and not o.x[bad].view(torch.int64).any()
    assert (o.base[bad] == -1).all() and not o.objrow[bad].view(torch.int64).any() and not o.row_width[bad].any()
    good = list(range(6))
    got = sx.BatchTensors(o.status[good], o.pivots[good], o.opt[good], o.x[good], o.base[good], o.objrow[good],
                          o.row_width[good], 0, None, None, gather(out, good))
    same_as_state_refs(got, want, n, m0 + 1)
    for src, data in zip(srcs, (A, b, c)):
        assert unchanged(src, data)
    same_state(state, keep)
    # the wrapper passes the same lists on
    res = sx.branch_batch_tensors(state, i32(parent), i32(var), f64(coef), f64(rhs), *tensors(insts), root=i32(root),
                                  objective_row=True)
    assert res.status.tolist() == o.status.tolist() and res.state.phase[bad].tolist() == [0] * 6
    same_as_state_refs(sx.BatchTensors(*(getattr(res, f)[good] for f in OUTPUTS), 0, None, None,
                                       gather(res.state, good)), want, n, m0 + 1)


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: every combination of the optional outputs NULL, with and without `out`"""
    n, m0 = 20, 10
    m = m0 + 1
    parent = PARENTS[1]
    insts, refs, tri, want = want_two_children(n, m0, parent, 0.5)
    C = len(parent)
    first, _ = kept(insts)
    keep = clone(first.state)
    A, b, c = tensors(insts)
    lists = (i32(parent), i32(tri[0]), f64(tri[1]), f64(tri[2]))
    names = ("x", "base", "objrow", "row_width")
    for case, nulls in enumerate(itertools.product((False, True), repeat=4)):
        kw = {name: None for name, null in zip(names, nulls) if null}
        out = sx.BatchState.empty(C, n, m, "cuda") if case % 2 == 0 or not any(nulls) else None
        o = branch_call(n, m, C, dense(A), dense(b), dense(c), first.state, len(insts), *lists, state_out=out, **kw)
        assert o.rc == 0 and int(o.evicted.item()) == 0
        assert all((getattr(o, name) is None) == null for name, null in zip(names, nulls))
        assert o.status.tolist() == [w["status"] for w in want]
        assert [tuple(p) for p in o.pivots.tolist()] == [w["pivots"] for w in want]
        assert np.array_equal(bits(o.opt.cpu().numpy()), bits([w["opt"] for w in want]))
        if o.x is not None:
            assert np.array_equal(bits(o.x.cpu().numpy()), bits(np.stack([w["x"] for w in want])))
        if o.base is not None:
            assert np.array_equal(o.base.cpu().numpy(), np.stack([w["base"] for w in want]))
        if o.row_width is not None:
            assert o.row_width.tolist() == [len(w["row"]) for w in want]
        if o.objrow is not None:
            rows = o.objrow.cpu().numpy()
            for k, w in enumerate(want):
                assert np.array_equal(bits(rows[k, :len(w["row"])]), bits(w["row"])), k
                assert not bits(rows[k, len(w["row"]):]).any(), k
        if out is not None:
            same_state(out, state_tensors(want))
    same_state(first.state, keep)  # nothing was written to `in`
