"""Rows or columns taken out of a kept batch state (simplex_solve_batch_device_drop, sx_batch.hip
k_batch_solve_drop) through sx.drop_rows_batch_tensors and sx.drop_cols_batch_tensors, and through a ctypes
caller (device_entries.drop_call) for what those never pass.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_drop_refs.py: the entry restated
from the oracle's argmin, ratio and pivot, batch_rhs_refs' dual loop and batch_state_refs._run
(test_batch_drop_host.py shows on the CPU what the restatement reaches, and which path each instance
takes).  Compared per problem: status, both pivot counts, the basis, objective and solution (NaN and zeros
unless FEASIBLE), the objective row and its width, and the whole reduced state: T, d, base, phase and
pivots.  In-states are solve_batch_tensors(keep_state=True) on generated instances in [1, 100]."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_cols_refs import ref_cols
from batch_drop_refs import (CAP_COLS, CAP_ROWS, COLS, DROP_CAPS, ROUND_TRIP_SHAPES, ROWS, added_col, added_row,
                             candidates, column_0_batch, forced_minus_instance, handmade, many_drops, mixed_batch,
                             reduced, ref_drop, shapes, want_batch)
from batch_refs import same_as_refs, same_tensors, tensors
from batch_rhs_refs import ref_rhs, ref_rhs_resume
from batch_rows_refs import make_row, ref_rows
from batch_state_refs import bits, ref_state, same_as_state_refs, state_tensors, warm_instances
from device_entries import dense, drop_call

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")
ROUNDING = 1e-10  # test_batch_drop_host.py


def kept(insts, max_pivots=-1):
    """one keep_state call, checked against the reference: (BatchTensors, refs)"""
    A, b, c = tensors(insts)
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, A.shape[2], A.shape[1])
    return out, refs


def index(lists):
    return torch.tensor([list(x) for x in lists], dtype=torch.int32, device="cuda")


def drop(state, kind, lists, small, **kw):
    """the rows or columns `lists` (one list per problem) taken out of `state`; small: the reduced instances"""
    A, b, c = tensors(small)
    fn = sx.drop_rows_batch_tensors if kind == ROWS else sx.drop_cols_batch_tensors
    out = fn(state, index(lists), A, b, c, objective_row=True, **kw)
    m, n = small[0][0].shape
    assert out.state is not state and out.state.rhs is True and (out.state.n, out.state.m) == (n, m)
    return out


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m, state.rhs)


def same_state(x, y, fields=STATE_FIELDS):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in fields:
        a, b = getattr(x, f), getattr(y, f)
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b), f


def shape_of(small):
    m, n = small[0][0].shape
    return n, m


# ------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("kind,shape", [(k, s) for k in (ROWS, COLS) for s in shapes(k)])
def test_shapes(gpu, kind, shape):
    """per shape a drop without arithmetic, a forced one and (q = 3) both in one list: the in-state's dense
    stride in both parities, the LDS class, the workspace class and the step from one to the other, the
    forced selections over two tiles and on either side of a tile's edge"""
    insts, refs, lists, small, want = want_batch(kind, *shape)
    first, _ = kept(insts)
    keep = clone(first.state)
    out = drop(first.state, kind, lists, small)
    assert out.evicted == 0
    same_as_state_refs(out, want, *shape_of(small))
    same_state(first.state, keep)


def test_forced_minus(gpu):
    """a batch of its own: the slack can only move down, the pivot element is negative"""
    inst = forced_minus_instance()
    first, refs = kept([inst])
    g = reduced(inst, ROWS, [0])
    want = ref_drop(refs[0], ROWS, [0], *g)
    assert want["paths"] == ["forced-"]
    same_as_state_refs(drop(first.state, ROWS, [[0]], [g]), [want], 2, 1)


@pytest.mark.parametrize("kind", [ROWS, COLS])
def test_no_candidate(gpu, kind):
    """hand-made states whose forced selection finds no candidate: cold, solve_batch_tensors on the reduced
    problem"""
    st, idx, g = handmade(kind)
    want = ref_drop(st, kind, idx, *g)
    assert want["why"] == "no-candidate"
    out = drop(state_tensors([st]), kind, [idx], [g])
    same_as_state_refs(out, [want], *shape_of([g]))
    plain = sx.solve_batch_tensors(*tensors([g]), objective_row=True)
    same_tensors(sx.BatchTensors(out.status, out.pivots, out.optimal_value, out.solution, out.base, out.objective_row,
                                 out.row_width, 0), plain)


# ------------------------------------------------------------------ round trips
@pytest.mark.parametrize("n,m", ROUND_TRIP_SHAPES)
def test_round_trips(gpu, n, m):
    """a loose cut added and dropped, a column that does not price in added and dropped: the kept T, d and
    base bit for bit; a binding cut added and dropped: the kept status, the optimum to the bound"""
    insts = warm_instances(n, m)[:3]
    first, refs = kept(insts)
    for theta in (1.5, 0.5):
        grown = [added_row(inst, theta) for inst in insts]
        mid = [ref_rows(r, *g) for r, g in zip(refs, grown)]
        one = sx.add_rows_batch_tensors(first.state, *tensors(grown), objective_row=True)
        same_as_state_refs(one, mid, n, m + 1)
        back = drop(one.state, ROWS, [[m]] * 3, insts)
        same_as_state_refs(back, [ref_drop(s, ROWS, [m], *inst) for s, inst in zip(mid, insts)], n, m)
        if theta > 1.0:
            same_state(back.state, first.state, ("T", "d", "base", "phase"))
            assert not back.pivots[:, 1].any()
        else:
            assert back.status.tolist() == first.status.tolist() == [sx.FEASIBLE] * 3
            assert ((back.optimal_value - first.optimal_value).abs() <= ROUNDING * first.optimal_value.abs()).all()
    grown = [added_col(inst, 0.01) for inst in insts]
    mid = [ref_cols(r, *g) for r, g in zip(refs, grown)]
    one = sx.add_cols_batch_tensors(first.state, *tensors(grown), objective_row=True)
    same_as_state_refs(one, mid, n + 1, m)
    back = drop(one.state, COLS, [[n]] * 3, insts)
    same_as_state_refs(back, [ref_drop(s, COLS, [n], *inst) for s, inst in zip(mid, insts)], n, m)
    same_state(back.state, first.state, ("T", "d", "base", "phase"))


# ------------------------------------------------------------------ cold and warm in one batch
@pytest.mark.parametrize("kind", [ROWS, COLS])
def test_mixed_states(gpu, kind):
    """phase-1 (INFEASIBLE), UNBOUNDED and FEASIBLE in-states in one call, every problem with its own
    index: the cold ones are solve_batch_tensors on the reduced problem"""
    insts = mixed_batch()
    first, refs = kept(insts)
    lists = [[k % (10 if kind == ROWS else 12)] for k in range(len(insts))]
    small = [reduced(inst, kind, idx) for inst, idx in zip(insts, lists)]
    want = [ref_drop(r, kind, idx, *g) for r, idx, g in zip(refs, lists, small)]
    cold = [k for k, w in enumerate(want) if w["why"]]
    assert {refs[k]["phase"] for k in cold} >= {1} and 0 < len(cold) < len(insts)
    assert {r["status"] for r in refs} >= {sx.INFEASIBLE, sx.UNBOUNDED, sx.FEASIBLE}
    out = drop(first.state, kind, lists, small)
    same_as_state_refs(out, want, *shape_of(small))
    plain = sx.solve_batch_tensors(*tensors(small), objective_row=True)
    pick = lambda o: sx.BatchTensors(*(t[cold] for t in (o.status, o.pivots, o.optimal_value, o.solution, o.base,  # noqa: E731
                                                          o.objective_row, o.row_width)), 0)
    same_tensors(pick(out), pick(plain))


# ------------------------------------------------------------------ phase-3 in-states
def test_phase_3_in_states(gpu):
    """test_batch_drop_host.py's cases: the impossible row stopped by a cap of 0 and the row 0 x <= -1
    dropped again (warm, basic slack, FEASIBLE again, the kept state bit for bit), the INFEASIBLE state's
    tight impossible row dropped (cold), a basic column dropped from a phase-3 state (warm)"""
    insts = warm_instances(12, 10)[:3]
    n, m = 12, 10
    first, refs = kept(insts)
    never = []
    for inst in insts:
        a, beta = make_row(inst, "never", 1.0)
        never.append((np.vstack([inst[0], a]), np.append(inst[1], beta), inst[2]))
    zero = [(np.vstack([inst[0], np.zeros(n)]), np.append(inst[1], -1.0), inst[2]) for inst in insts]
    for grown, cap, warm in ((never, 0, True), (zero, -1, True), (never, -1, False)):
        mid = [ref_rows(r, *g, cap) for r, g in zip(refs, grown)]
        assert all(s["phase"] == 3 for s in mid)
        stuck = sx.add_rows_batch_tensors(first.state, *tensors(grown), max_pivots=cap, objective_row=True)
        same_as_state_refs(stuck, mid, n, m + 1)
        want = [ref_drop(s, ROWS, [m], *inst) for s, inst in zip(mid, insts)]
        assert all((w["why"] is None) == warm for w in want)
        back = drop(stuck.state, ROWS, [[m]] * 3, insts)
        same_as_state_refs(back, want, n, m)
        assert back.status.tolist() == [sx.FEASIBLE] * 3
        if warm:
            same_state(back.state, first.state, ("T", "d", "base", "phase"))
    cut = [added_row(inst, 0.5) for inst in insts]
    mid = [ref_rows(r, *g, 0) for r, g in zip(refs, cut)]
    stuck = sx.add_rows_batch_tensors(first.state, *tensors(cut), max_pivots=0, objective_row=True)
    same_as_state_refs(stuck, mid, n, m + 1)
    lists = [[candidates(s, COLS)[1][0]] for s in mid]
    small = [reduced(g, COLS, idx) for g, idx in zip(cut, lists)]
    want = [ref_drop(s, COLS, idx, *g) for s, idx, g in zip(mid, lists, small)]
    assert all(w["paths"] == ["forced-dual"] and w["dual"] >= 1 for w in want)
    same_as_state_refs(drop(stuck.state, COLS, lists, small), want, n - 1, m + 1)


def test_a_column_whose_removal_is_infeasible(gpu):
    """-x_0 <= -1 among the rows, column 0 dropped: INFEASIBLE, found in the dual loop where x_0 > 1 stands
    in another row and cold where the row itself holds it (test_batch_drop_host.py), as from scratch"""
    big = column_0_batch()
    first, refs = kept(big)
    small = [reduced(g, COLS, [0]) for g in big]
    want = [ref_drop(r, COLS, [0], *g) for r, g in zip(refs, small)]
    assert all(w["status"] == sx.INFEASIBLE for w in want)
    assert [w["path"] for w in want] == ["cold", "forced-dual", "forced-dual"] and want[1]["phase"] == 3
    out = drop(first.state, COLS, [[0]] * 3, small)
    same_as_state_refs(out, want, 11, 11)
    assert sx.solve_batch_tensors(*tensors(small)).status.tolist() == [sx.INFEASIBLE] * 3


# ------------------------------------------------------------------ cap, budget
@pytest.mark.parametrize("cap", DROP_CAPS)
@pytest.mark.parametrize("kind", [ROWS, COLS])
def test_cap_behind_the_forced_pivots_and_resume(gpu, kind, cap):
    shape = CAP_ROWS if kind == ROWS else CAP_COLS
    insts, refs, lists, small, whole = want_batch(kind, *shape)
    crefs = want_batch(kind, *shape, cap)[4]
    first, _ = kept(insts)
    capped = drop(first.state, kind, lists, small, max_pivots=cap)
    same_as_state_refs(capped, crefs, *shape_of(small))
    if cap < 4:
        assert sx.PIVOT_CAP in capped.status.tolist()
    keep = clone(capped.state)
    done = sx.resume_batch_tensors(capped.state, tensors(small)[2], objective_row=True, in_place=False)
    assert done.state.rhs is True and done.evicted == 0
    same_as_state_refs(done, whole, *shape_of(small))
    same_state(capped.state, keep)


def test_budget_behind_the_forced_pivots(gpu):
    """a resident budget of 2 pivots per call does not count the forced pivot: a problem with more than
    f + 2 pivots is evicted with the state a cap of f + 2 leaves, and every plain resume takes it further,
    until nothing is evicted"""
    insts, refs, lists, small, whole = want_batch(ROWS, *CAP_ROWS)
    first, _ = kept(insts)
    c = tensors(small)[2]
    long = [k for k, w in enumerate(whole) if w["pivots"][1] > w["forced"] + 2]
    assert len(long) >= 2
    sx.set_batch_budget(2)
    try:
        out = drop(first.state, ROWS, lists, small)
        assert out.evicted == len(long)
        for k in long:
            cap = ref_drop(refs[k], ROWS, lists[k], *small[k], whole[k]["forced"] + 2)
            assert out.status[k].item() == sx.NOT_ENDED and out.pivots[k, 1].item() == whole[k]["forced"] + 2
            assert np.array_equal(bits(out.state.T[k].cpu().numpy()), bits(cap["T"]))
            assert np.array_equal(out.state.base[k].cpu().numpy(), cap["base"])
        calls = 0
        while out.evicted:
            calls += 1
            assert calls <= 8, "an evicted problem does not progress"
            out = sx.resume_batch_tensors(out.state, c, objective_row=True)
    finally:
        sx.set_batch_budget(0)
    assert calls >= 1
    same_as_state_refs(out, whole, *shape_of(small))


# ------------------------------------------------------------------ a chain
def test_row_column_drop_rhs_drop(gpu):
    """a row added, a column added, that row dropped, a new right-hand side, that column dropped: every
    entry takes the state the one before it left"""
    n, m = 32, 16
    insts = warm_instances(n, m)[:3]
    first, refs = kept(insts)
    g1 = [added_row(inst, 0.5) for inst in insts]
    w1 = [ref_rows(r, *g) for r, g in zip(refs, g1)]
    s1 = sx.add_rows_batch_tensors(first.state, *tensors(g1), objective_row=True)
    same_as_state_refs(s1, w1, n, m + 1)
    g2 = [added_col(g, 100.0) for g in g1]
    w2 = [ref_cols(w, *g) for w, g in zip(w1, g2)]
    s2 = sx.add_cols_batch_tensors(s1.state, *tensors(g2), objective_row=True)
    same_as_state_refs(s2, w2, n + 1, m + 1)
    g3 = [reduced(g, ROWS, [m]) for g in g2]
    w3 = [ref_drop(w, ROWS, [m], *g) for w, g in zip(w2, g3)]
    s3 = drop(s2.state, ROWS, [[m]] * 3, g3)
    same_as_state_refs(s3, w3, n + 1, m)
    g4 = [(g[0], 1.05 * g[1], g[2]) for g in g3]
    w4 = [ref_rhs(w, *g) for w, g in zip(w3, g4)]
    A4, b4, c4 = tensors(g4)
    s4 = sx.resume_batch_tensors(s3.state, c4, objective_row=True, in_place=False, A=A4, b=b4)
    same_as_state_refs(s4, w4, n + 1, m)
    g5 = [reduced(g, COLS, [n]) for g in g4]
    w5 = [ref_drop(w, COLS, [n], *g) for w, g in zip(w4, g5)]
    s5 = drop(s4.state, COLS, [[n]] * 3, g5)
    same_as_state_refs(s5, w5, n, m)
    assert {p for w in w3 + w5 for p in w["paths"]} >= {"forced+"}


# ------------------------------------------------------------------ strides, many problems, a stream
def test_strided_b_and_transposed_a(gpu):
    """warm (nothing of A, b, c is read) and cold (the reduced problem is read through its strides)"""
    kind, shape = ROWS, (20, 11, 1)
    insts, refs, lists, small, want = want_batch(kind, *shape)
    n, m = shape_of(small)
    A, b, c = tensors(small)
    wide = torch.full((3, 2 * m + 3), 7.0, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * m + 1:2] = b
    view = wide[:, 1:2 * m + 1:2]
    assert view.stride() == (2 * m + 3, 2)
    At = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert At.stride() == (n * m, 1, m)
    first, _ = kept(insts)
    out = sx.drop_rows_batch_tensors(first.state, index(lists)[:, :1], At, view, c, objective_row=True)
    same_as_state_refs(out, want, n, m)
    cold = state_tensors([ref_state(*inst, 2) for inst in insts])
    assert cold.phase.tolist() == [1] * 3
    # the index tensor is made dense by the wrapper: a strided view of a wider one
    two = torch.stack([index(lists)[:, 0], index(lists)[:, 0]], dim=1)[:, 1:]
    assert not two.is_contiguous()
    out = sx.drop_rows_batch_tensors(cold, two, At, view, c, objective_row=True)
    same_as_state_refs(out, [ref_state(*g) for g in small], n, m)


def test_more_problems_than_resident_workgroups(gpu):
    """1,200 problems of (5, 5 -> 4), each dropping its own row"""
    insts = many_drops()
    assert len(insts) == 1200
    first, refs = kept(insts)
    lists = [[k % 5] for k in range(1200)]
    small = [reduced(inst, ROWS, idx) for inst, idx in zip(insts, lists)]
    want = [ref_drop(r, ROWS, idx, *g) for r, idx, g in zip(refs, lists, small)]
    assert sum(w["forced"] for w in want) >= 100 and sum(w["path"] == "none" for w in want) >= 100
    same_as_state_refs(drop(first.state, ROWS, lists, small), want, 5, 4)


def test_non_default_stream(gpu):
    insts, refs, lists, small, whole = want_batch(ROWS, *CAP_ROWS)
    first, _ = kept(insts)
    A, b, c = tensors(small)
    idx = index(lists)
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        capped = sx.drop_rows_batch_tensors(first.state, idx, A, b, c, max_pivots=2, objective_row=True, finish=False)
        done = sx.resume_batch_tensors(capped.state, c, objective_row=True, finish=False, in_place=False)
    s0.synchronize()
    assert isinstance(done.evicted, torch.Tensor) and int(done.evicted.item()) == 0
    same_as_state_refs(capped, want_batch(ROWS, *CAP_ROWS, 2)[4], *shape_of(small))
    same_as_state_refs(done, whole, *shape_of(small))


# ------------------------------------------------------------------ bad inputs
def test_bad_inputs_beside_a_good_problem(gpu):
    """a descending list, a repeated index, an index equal to m_in, phase 0 and a negative pivot count:
    BAD_STATE, cleared outputs and phase 0 for that problem alone"""
    n, m_in = 20, 11
    base = want_batch(ROWS, n, m_in, 1)[0]
    insts = [base[k % 3] for k in range(6)]
    first, refs = kept(insts)
    state = clone(first.state)
    lists = [[3, 1], [2, 2], [4, m_in], [1, 4], [1, 4], [1, 4]]
    state.phase[3] = 0
    state.pivots[4, 1] = -1
    small = [reduced(inst, ROWS, [1, 4]) for inst in insts]
    out = drop(state, ROWS, lists, small)
    bad = [0, 1, 2, 3, 4]
    assert out.status.tolist() == [sx.BAD_STATE] * 5 + [refs[5]["status"]]
    assert out.state.phase.tolist() == [0] * 5 + [2] and not out.pivots[bad].any()
    assert torch.isnan(out.optimal_value[bad]).all() and not out.solution[bad].view(torch.int64).any()
    assert (out.base[bad] == -1).all() and not out.objective_row[bad].view(torch.int64).any()
    assert not out.row_width[bad].any()
    good = sx.BatchTensors(*(t[5:] for t in (out.status, out.pivots, out.optimal_value, out.solution, out.base,
                                              out.objective_row, out.row_width)), 0)
    same_as_refs(good, [ref_drop(refs[5], ROWS, [1, 4], *small[5])], n, m_in - 2)
    # columns: an index equal to n_in beside a good problem
    out = drop(first.state, COLS, [[n]] + [[0]] * 5, [reduced(inst, COLS, [0]) for inst in insts])
    assert out.status.tolist()[0] == sx.BAD_STATE and sx.BAD_STATE not in out.status.tolist()[1:]


# ------------------------------------------------------------------ C-only cases
def test_c_caller_null_arguments(gpu):
    """through ctypes: `out` NULL and every optional output NULL; then into a state with the outputs; a
    negative count; a workspace sized for the reduced shape where the in-state's is of the workspace class"""
    insts, refs, lists, small, whole = want_batch(ROWS, *CAP_ROWS)
    n, m = shape_of(small)
    B = len(insts)
    first, _ = kept(insts)
    A, b, c = tensors(small)
    idx = index(lists)
    keep = clone(first.state)
    o = drop_call(n, m, B, dense(A), dense(b), dense(c), first.state, ROWS, idx, x=None, base=None, objrow=None,
                  row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(first.state, keep)  # nothing was written to `in`
    assert o.status.tolist() == [r["status"] for r in whole]
    assert [tuple(q) for q in o.pivots.tolist()] == [r["pivots"] for r in whole]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([r["opt"] for r in whole]))
    assert int(o.evicted.item()) == 0
    capped = sx.BatchState.empty(B, n, m, "cuda")
    o = drop_call(n, m, B, dense(A), dense(b), dense(c), first.state, ROWS, idx, state_out=capped, max_pivots=2)
    assert o.rc == 0
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, capped)
    crefs = want_batch(ROWS, *CAP_ROWS, 2)[4]
    same_as_state_refs(got, crefs, n, m)
    capped.rhs = True
    done = sx.resume_batch_tensors(capped, c, objective_row=True)
    same_as_state_refs(done, [ref_rhs_resume(r, g[2]) for r, g in zip(crefs, small)], n, m)
    same_as_state_refs(done, whole, n, m)
    assert drop_call(n, m, B, dense(A), dense(b), dense(c), first.state, ROWS, idx, call_count=-1).rc == -1
    # (241, 64) works in a workspace slice, the reduced (241, 63) is of the LDS class: its header alone is too small
    assert sx.batch_class(241, 64) == 1 and sx.batch_class(n, m) == 2
    assert drop_call(n, m, B, dense(A), dense(b), dense(c), first.state, ROWS, idx, ws_shape=(n, m)).rc == -5
