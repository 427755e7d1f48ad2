"""Gomory mixed-integer cuts from a kept batch state (simplex_solve_batch_device_cut, sx_batch.hip
k_batch_solve_cut) through sx.cut_batch_tensors, and through a ctypes caller (device_entries.cut_call) for what
that never passes.  Needs an MI355X.

Everything is compared bit for bit, without a tolerance, against batch_cut_refs.py: the entry restated from
batch_rows_refs.ref_rows, the oracle's eps-argmin tree and the oracle's fma (test_batch_cut_host.py shows on
the CPU what the restatement reaches).  Compared per problem: the emitted rows cut_A and cut_b where the
caller's A and b were overwritten, cut_rows, status, both pivot counts, the basis, objective and solution,
the objective row and its width, and the whole grown state: T, d, base, phase and pivots."""
import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from batch_cut_refs import AWAY, SCALES, cut_instances, grown_arrays, masks, mixed_cut_instances, ref_cut, row_keys
from batch_refs import same_as_refs, same_tensors, tensors
from batch_rhs_refs import DBL_MAX, ref_rhs, ref_rhs_resume, scaled_rhs
from batch_rows_refs import lds_edge, rows_shapes
from batch_state_refs import bits, many_instances, ref_state, same_as_state_refs, state_tensors
from device_entries import SENTINEL, cut_call, dense

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("T", "d", "base", "phase", "pivots")
FILL = 7.0  # what the rows reserved for the cuts hold before the call


def kept(insts, max_pivots=-1):
    """one keep_state call, checked against the reference: (BatchTensors, refs)"""
    A, b, c = tensors(insts)
    m, n = insts[0][0].shape
    out = sx.solve_batch_tensors(A, b, c, max_pivots=max_pivots, objective_row=True, keep_state=True)
    refs = [ref_state(*inst, max_pivots) for inst in insts]
    same_as_state_refs(out, refs, n, m)
    return out, refs


def envelope(insts, q):
    """A [B, m0 + q, n] and b [B, m0 + q] whose first m0 rows are the instances' and whose last q hold FILL,
    and c"""
    A0, b0, c = tensors(insts)
    B, m0, n = A0.shape
    A = torch.full((B, m0 + q, n), FILL, dtype=torch.float64, device="cuda")
    b = torch.full((B, m0 + q), FILL, dtype=torch.float64, device="cuda")
    A[:, :m0] = A0
    b[:, :m0] = b0
    return A, b, c


def refs_of(states, insts, mask, q, rows=None, max_pivots=-1):
    """ref_cut per problem; mask [n] for all or [B, n], rows None or [B, q]"""
    mask = np.asarray(mask)
    return [ref_cut(st, inst[0], inst[1], inst[2], mask if mask.ndim == 1 else mask[k], q, AWAY,
                    None if rows is None else rows[k], max_pivots) for k, (st, inst) in enumerate(zip(states, insts))]


def same_cuts(A, b, cut_rows, want, m0):
    """rows m0 .. m of the caller's A and b and cut_rows against ref_cut's, bit for bit"""
    A, b, cut_rows = A.cpu().numpy(), b.cpu().numpy(), cut_rows.cpu().numpy()
    assert cut_rows.dtype == np.int32 and cut_rows.shape == (len(want), A.shape[1] - m0)
    for k, (cut_A, cut_b, cut_row, _) in enumerate(want):
        assert np.array_equal(cut_rows[k], cut_row), k
        assert np.array_equal(bits(A[k, m0:]), bits(cut_A)), k
        assert np.array_equal(bits(b[k, m0:]), bits(cut_b)), k


def cut(state, insts, want, q, mask, **kw):
    """sx.cut_batch_tensors into a fresh envelope, compared with `want` in every field; returns (out, A, b)"""
    A, b, c = envelope(insts, q)
    m0, n = insts[0][0].shape
    src = (A[:, :m0].clone(), b[:, :m0].clone())
    out = sx.cut_batch_tensors(state, A, b, c, torch.as_tensor(np.asarray(mask)).cuda(), cuts=q, objective_row=True, **kw)
    assert out.state is not state and out.state.rhs is True and (out.state.n, out.state.m) == (n, m0 + q)
    assert torch.equal(A[:, :m0].view(torch.int64), src[0].view(torch.int64))  # the source rows are only read
    assert torch.equal(b[:, :m0].view(torch.int64), src[1].view(torch.int64))
    same_cuts(A, b, out.cut_rows, want, m0)
    same_as_state_refs(out, [w[3] for w in want], n, m0 + q)
    return out, A, b


def clone(state):
    return sx.BatchState(*(getattr(state, f).clone() for f in STATE_FIELDS), state.n, state.m, state.rhs)


def same_state(x, y):
    """two BatchStates bit for bit"""
    assert (x.n, x.m) == (y.n, y.m)
    for f in ("base", "phase", "pivots"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f


def real(want):
    """real cuts per problem"""
    return [int((w[2] >= 0).sum()) for w in want]


# ------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("n,m0,q", rows_shapes())
def test_shapes(gpu, n, m0, q):
    """both scales of b, all-integer mask, on every shape: the in-state's dense stride in both parities, q = 3
    with a null row behind real ones, the LDS class, the workspace class and the step from one to the other
    (an LDS state read by a workspace-class launch), g and the chain over two column tiles ((241, 64) in the
    slack part, (4, 512) too, (600, 4) in the structural part and in the caller's variables)"""
    got = 0
    for scale in SCALES:
        insts = cut_instances(n, m0, scale)
        first, refs = kept(insts)
        keep = clone(first.state)
        want = refs_of(refs, insts, masks(n)["all"], q)
        got += sum(real(want))
        out, _, _ = cut(first.state, insts, want, q, masks(n)["all"])
        assert out.evicted == 0
        same_state(first.state, keep)
    assert got >= 1


# ------------------------------------------------------------------ the row choice over two row tiles
def _permuted(state, perm):
    """the kept state with its rows in another order: T's rows and the basis together (a row permutation of
    a kept state is a kept state of the same problem)"""
    out = dict(state)
    out["T"] = np.ascontiguousarray(state["T"][perm])
    out["base"] = np.ascontiguousarray(state["base"][perm])
    return out


@pytest.mark.parametrize("winner_last", [True, False])
def test_row_choice_across_two_row_tiles(gpu, winner_last):
    """(4, 513): the keys fill two tiles of the argmin.  The winning eligible row is row 512, alone in the
    second tile, with the runner-up in the first tile -- and the other way round"""
    n, m0 = 4, 513
    assert sx.batch_class(n, m0 + 1) == 1
    insts, states = [], []
    for inst in cut_instances(n, m0, 37):
        st = ref_state(*inst)
        keys = row_keys(st, masks(n)["all"], AWAY)
        order = np.argsort(keys, kind="stable")
        if keys[order[1]] == DBL_MAX or keys[order[1]] - keys[order[0]] < 1e-6:
            continue  # fewer than two eligible rows, or no clear winner
        best, second = int(order[0]), int(order[1])
        hi, lo = (best, second) if winner_last else (second, best)
        perm = [i for i in range(m0) if i not in (best, second)]
        perm.insert(5, lo)
        perm.append(hi)
        assert len(perm) == m0 and perm[5] == lo and perm[512] == hi
        insts.append(inst)
        states.append(_permuted(st, perm))
    assert insts
    want = refs_of(states, insts, masks(n)["all"], 1)
    assert all(w[2][0] == (512 if winner_last else 5) for w in want)
    cut(state_tensors(states), insts, want, 1, masks(n)["all"])


# ------------------------------------------------------------------ q = 3
@pytest.mark.parametrize("n,m0", [(5, 4), (33, 31), (241, 64)])
def test_three_cuts(gpu, n, m0):
    """three cuts in one call come from three different source rows; at (5, 4) fewer than three rows are
    eligible, so a null row stands behind the real ones"""
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(n)["all"], 3)
    counts = real(want)
    if (n, m0) == (5, 4):
        assert 0 < max(counts) < 3
    else:
        assert max(counts) == 3
    for w in want:
        rows = w[2][w[2] >= 0]
        assert len(set(rows.tolist())) == len(rows) and (w[2][len(rows):] == -1).all()
    cut(first.state, insts, want, 3, masks(n)["all"])


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("n,m0", [(20, 10), (33, 31)])
def test_two_rounds(gpu, n, m0):
    """round one's out-state and the A and b it overwrote feed round two: a source row of round two has a
    non-zero g on the first cut's slack, which is substituted through the first cut's row"""
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    want1 = refs_of(refs, insts, masks(n)["all"], 1)
    one, A1, b1 = cut(first.state, insts, want1, 1, masks(n)["all"])
    grown = [grown_arrays(inst, w) for inst, w in zip(insts, want1)]
    states = [w[3] for w in want1]
    want2 = refs_of(states, grown, masks(n)["all"], 1)
    assert sum(real(want2)) >= 1
    # a cut slack that is nonbasic in a source row of round two
    assert any(w[2][0] >= 0 and st["T"][w[2][0], 1 + n + m0] != 0.0 and n + m0 not in st["base"]
               for st, w in zip(states, want2))
    # the tensors round one wrote are round two's source, with one more row reserved
    A2 = torch.full((len(insts), m0 + 2, n), FILL, dtype=torch.float64, device="cuda")
    b2 = torch.full((len(insts), m0 + 2), FILL, dtype=torch.float64, device="cuda")
    A2[:, :m0 + 1] = A1
    b2[:, :m0 + 1] = b1
    c = tensors(insts)[2]
    two = sx.cut_batch_tensors(one.state, A2, b2, c, torch.ones(n, dtype=torch.bool, device="cuda"), objective_row=True)
    same_cuts(A2, b2, two.cut_rows, want2, m0 + 1)
    same_as_state_refs(two, [w[3] for w in want2], n, m0 + 2)


def test_cut_then_new_rhs_then_cut(gpu):
    """the grown state is a state of the right-hand-side entry: a new b [m] on it, then another cut"""
    n, m0 = 20, 10
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    want1 = refs_of(refs, insts, masks(n)["all"], 1)
    one, A1, b1 = cut(first.state, insts, want1, 1, masks(n)["all"])
    grown = [grown_arrays(inst, w) for inst, w in zip(insts, want1)]
    b2s = [scaled_rhs(g[1], 1000 + k, 0.1) for k, g in enumerate(grown)]
    want2 = [ref_rhs(w[3], g[0], b2, g[2]) for w, g, b2 in zip(want1, grown, b2s)]
    c = tensors(insts)[2]
    b2 = torch.from_numpy(np.stack(b2s)).cuda()
    two = sx.resume_batch_tensors(one.state, c, objective_row=True, in_place=False, A=A1, b=b2)
    same_as_state_refs(two, want2, n, m0 + 1)
    moved = [(g[0], b2k, g[2]) for g, b2k in zip(grown, b2s)]
    want3 = refs_of(want2, moved, masks(n)["all"], 1)
    cut(two.state, moved, want3, 1, masks(n)["all"])


# ------------------------------------------------------------------ the caller's rows
def test_rows_given_by_the_caller(gpu):
    """per problem: the kernel's own choice passed back in (the same cut), then an ineligible row (a basic
    slack's, or any row under a mask that excludes its variable), an index out of range on either side, and
    a duplicate of the first cut's row: the last three give null rows"""
    n, m0, q = 33, 31, 2
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    own = refs_of(refs, insts, masks(n)["all"], q)
    assert all(r == 2 for r in real(own))
    chosen = np.stack([w[2] for w in own])
    back = refs_of(refs, insts, masks(n)["all"], q, rows=chosen)
    for w, v in zip(own, back):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(w[:2], v[:2])) and np.array_equal(w[2], v[2])
    cut(first.state, insts, back, q, masks(n)["all"], rows=torch.from_numpy(chosen).cuda())
    slack_rows = [int(np.flatnonzero(r["base"] >= n)[0]) for r in refs]
    for second in (slack_rows, [m0] * 3, [-1] * 3, [2 ** 30] * 3, chosen[:, 0].tolist()):
        rows = np.stack([chosen[:, 0], np.array(second)], axis=1).astype(np.int32)
        want = refs_of(refs, insts, masks(n)["all"], q, rows=rows)
        assert all(w[2][0] >= 0 and w[2][1] == -1 for w in want), second
        cut(first.state, insts, want, q, masks(n)["all"], rows=torch.from_numpy(rows).cuda())


# ------------------------------------------------------------------ masks
def test_masks(gpu):
    """one [n] mask for every problem (batch stride 0), as bool and as uint8; a [B, n] mask that differs per
    problem; and the none mask, which makes every cut null: add_rows_batch_tensors with rows of zeros"""
    n, m0 = 20, 10
    insts = cut_instances(n, m0, 37) + cut_instances(n, m0, 1)
    first, refs = kept(insts)
    second = masks(n)["second"]
    want = refs_of(refs, insts, second, 1)
    cut(first.state, insts, want, 1, second)
    cut(first.state, insts, want, 1, second.astype(np.uint8))
    per = np.stack([np.roll(second, k) if k % 3 else masks(n)["all"] for k in range(len(insts))])
    want = refs_of(refs, insts, per, 1)
    assert sum(real(want)) >= 2 and len({tuple(w[2]) for w in want}) >= 2
    cut(first.state, insts, want, 1, per)
    cut(first.state, insts, want, 1, per.astype(np.uint8) * 3)  # any non-zero byte
    want = refs_of(refs, insts, masks(n)["none"], 2)
    assert real(want) == [0] * len(insts)
    out, A, b = cut(first.state, insts, want, 2, masks(n)["none"])
    assert not A[:, m0:].view(torch.int64).any() and not b[:, m0:].view(torch.int64).any()
    plain = sx.add_rows_batch_tensors(first.state, A.clone(), b.clone(), tensors(insts)[2], objective_row=True)
    same_tensors(out, plain)
    same_state(out.state, plain.state)


# ------------------------------------------------------------------ states that are not kept optima
def test_mixed_states(gpu):
    """phase-1 (INFEASIBLE), UNBOUNDED and FEASIBLE states in one call: only the kept optima are cut, and the
    cold problems are solve_batch_tensors on the problem with null rows"""
    insts = mixed_cut_instances()
    m0, n = insts[0][0].shape
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(n)["all"], 1)
    cold = [k for k, w in enumerate(want) if "dual" not in w[3]]
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold} == {(1, sx.INFEASIBLE), (2, sx.UNBOUNDED)}
    assert 0 < len(cold) < len(insts) and all(want[k][2][0] == -1 for k in cold)
    out, A, b = cut(first.state, insts, want, 1, masks(n)["all"])
    plain = sx.solve_batch_tensors(A, b, tensors(insts)[2], objective_row=True)
    pick = lambda o: sx.BatchTensors(*(t[cold] for t in (o.status, o.pivots, o.optimal_value, o.solution, o.base,  # noqa: E731
                                                          o.objective_row, o.row_width)), 0)
    same_tensors(pick(out), pick(plain))


def test_phase_3_state_gets_a_null_row(gpu):
    """states that a capped cut left inside the dual loop are not kept optima: a null row, and the dual loop
    continues from pivot 0 on the grown tableau, as the rows entry does with a row of zeros"""
    n, m0 = 241, lds_edge(241)
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    capped = refs_of(refs, insts, masks(n)["all"], 1, max_pivots=1)
    assert [w[3]["phase"] for w in capped] == [3] * 3
    one, A1, b1 = cut(first.state, insts, capped, 1, masks(n)["all"], max_pivots=1)
    grown = [grown_arrays(inst, w) for inst, w in zip(insts, capped)]
    want = refs_of([w[3] for w in capped], grown, masks(n)["all"], 1)
    assert real(want) == [0] * 3 and any(w[3]["dual"] >= 1 for w in want)
    cut(one.state, grown, want, 1, masks(n)["all"])


@pytest.mark.parametrize("cap", [1, 2])
def test_cap_inside_the_dual_loop_and_resume(gpu, cap):
    """a cap inside the dual loop behind the cut, resumed through resume_batch_tensors: the uncapped call"""
    n, m0 = 241, lds_edge(241)
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    whole = refs_of(refs, insts, masks(n)["all"], 1)
    crefs = refs_of(refs, insts, masks(n)["all"], 1, max_pivots=cap)
    stopped = [w[3]["status"] == sx.PIVOT_CAP and w[3]["phase"] == 3 and w[3]["pivots"][1] == cap for w in crefs]
    # (the loop tests the cap before it tests the column, so a loop that needs exactly `cap` pivots stops too)
    assert any(stopped) and all(s == (w[3]["dual"] >= cap) for s, w in zip(stopped, whole))
    capped, _, _ = cut(first.state, insts, crefs, 1, masks(n)["all"], max_pivots=cap)
    done = sx.resume_batch_tensors(capped.state, tensors(insts)[2], objective_row=True, in_place=False)
    assert done.state.rhs is True and done.evicted == 0
    same_as_state_refs(done, [w[3] for w in whole], n, m0 + 1)
    same_as_state_refs(done, [ref_rhs_resume(w[3], inst[2]) for w, inst in zip(crefs, insts)], n, m0 + 1)


# ------------------------------------------------------------------ strides, many problems, a stream
def test_strides_and_envelope(gpu):
    """A transposed in memory, b strided, and A a view into a taller envelope: the rows beyond m, the gaps of
    the strided b and what lies around both stay untouched; the cold path reads through the strides too"""
    n, m0, q = 20, 10, 2
    m = m0 + q
    insts = cut_instances(n, m0, 37)
    B = len(insts)
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(n)["all"], q)
    A0, b0, c = tensors(insts)
    mask = torch.ones(n, dtype=torch.bool, device="cuda")

    def views():
        tall = torch.full((B, n, m + 3), SENTINEL, dtype=torch.float64, device="cuda")  # [B, n, rows]: transposed
        A = tall.transpose(1, 2)[:, :m]
        assert A.stride() == (n * (m + 3), 1, m + 3) and tuple(A.shape) == (B, m, n)
        A[:, :m0] = A0
        A[:, m0:] = FILL
        wide = torch.full((B, 2 * m + 3), SENTINEL, dtype=torch.float64, device="cuda")
        b = wide[:, 1:2 * m + 1:2]
        assert b.stride() == (2 * m + 3, 2)
        b[:, :m0] = b0
        b[:, m0:] = FILL
        return tall, A, wide, b

    def untouched(tall, wide):
        assert (tall[:, :, m:] == SENTINEL).all()  # the envelope's rows beyond m
        assert (wide[:, 0::2] == SENTINEL).all() and (wide[:, 2 * m + 1:] == SENTINEL).all()

    tall, A, wide, b = views()
    out = sx.cut_batch_tensors(first.state, A, b, c, mask, cuts=q, objective_row=True)
    same_cuts(A, b, out.cut_rows, want, m0)
    same_as_state_refs(out, [w[3] for w in want], n, m)
    untouched(tall, wide)
    assert torch.equal(A[:, :m0], A0) and torch.equal(b[:, :m0], b0)
    # phase-1 states: cold, null rows
    cold_refs = [ref_state(*inst, 2) for inst in insts]
    assert [r["phase"] for r in cold_refs] == [1] * 3
    cold_want = refs_of(cold_refs, insts, masks(n)["all"], q)
    tall, A, wide, b = views()
    out = sx.cut_batch_tensors(state_tensors(cold_refs), A, b, c, mask, cuts=q, objective_row=True)
    same_cuts(A, b, out.cut_rows, cold_want, m0)
    same_as_state_refs(out, [w[3] for w in cold_want], n, m)
    untouched(tall, wide)


def test_more_problems_than_resident_workgroups(gpu):
    insts = [(A, b * 37.0, c) for A, b, c in many_instances()]
    assert len(insts) == 1200
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(5)["all"], 1)
    assert sum(real(want)) >= 600
    cut(first.state, insts, want, 1, masks(5)["all"])


def test_non_default_stream(gpu):
    n, m0 = 33, 31
    insts = cut_instances(n, m0, 37)
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(n)["all"], 1)
    A, b, c = envelope(insts, 1)
    mask = torch.ones(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()  # the inputs are complete before the side stream reads them
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        out = sx.cut_batch_tensors(first.state, A, b, c, mask, objective_row=True, finish=False)
    s0.synchronize()
    assert isinstance(out.evicted, torch.Tensor) and int(out.evicted.item()) == 0
    same_cuts(A, b, out.cut_rows, want, m0)
    same_as_state_refs(out, [w[3] for w in want], n, m0 + 1)


# ------------------------------------------------------------------ bad states
def test_bad_states(gpu):
    """a base entry that the grown shape would accept but the in-state's does not, phase 0 and a negative
    pivot count: BAD_STATE, cleared outputs, phase 0, cut_rows -1 and rows of +0.0 for that problem alone"""
    n, m0 = 20, 10
    insts = cut_instances(n, m0, 37) + cut_instances(n, m0, 37)[2:]
    first, refs = kept(insts)
    state = clone(first.state)
    state.base[0, 3] = n + m0       # < n + m0 + 1: the new row's own slack, not a variable of the in-state
    state.phase[1] = 0
    state.pivots[2, 1] = -1
    A, b, c = envelope(insts, 1)
    out = sx.cut_batch_tensors(state, A, b, c, torch.ones(n, dtype=torch.bool, device="cuda"), objective_row=True)
    bad = [0, 1, 2]
    assert out.status.tolist() == [sx.BAD_STATE] * 3 + [sx.FEASIBLE]
    assert out.state.phase.tolist() == [0] * 3 + [2] and not out.pivots[bad].any()
    assert torch.isnan(out.optimal_value[bad]).all() and not out.solution[bad].view(torch.int64).any()
    assert (out.base[bad] == -1).all() and not out.objective_row[bad].view(torch.int64).any()
    assert not out.row_width[bad].any()
    assert (out.cut_rows[bad] == -1).all()
    assert not A[bad, m0:].view(torch.int64).any() and not b[bad, m0:].view(torch.int64).any()
    want = refs_of(refs[3:], insts[3:], masks(n)["all"], 1)
    assert real(want) == [1]
    same_cuts(A[3:], b[3:], out.cut_rows[3:], want, m0)
    good = sx.BatchTensors(*(t[3:] for t in (out.status, out.pivots, out.optimal_value, out.solution, out.base,
                                              out.objective_row, out.row_width)), 0)
    same_as_refs(good, [want[0][3]], n, m0 + 1)


# ------------------------------------------------------------------ C-only cases
def test_c_caller(gpu):
    """through ctypes: cut_A and cut_b in dense buffers of their own (the source holds m0 rows and no more),
    `out` NULL and every optional output NULL; then into a state with the outputs"""
    n, m0, q = 33, 31, 2
    m = m0 + q
    insts = cut_instances(n, m0, 37)
    B = len(insts)
    first, refs = kept(insts)
    want = refs_of(refs, insts, masks(n)["all"], q)
    A0, b0, c = tensors(insts)
    mask = torch.ones((B, n), dtype=torch.uint8, device="cuda")
    keep = clone(first.state)

    def same_own(o):
        assert np.array_equal(o.cut_row.cpu().numpy(), np.stack([w[2] for w in want]))
        assert np.array_equal(bits(o.cut_A.cpu().numpy()), bits(np.stack([w[0] for w in want])))
        assert np.array_equal(bits(o.cut_b.cpu().numpy()), bits(np.stack([w[1] for w in want])))

    o = cut_call(n, m, B, dense(A0), dense(b0), dense(c), first.state, mask, cuts=q, x=None, base=None, objrow=None,
                 row_width=None)
    assert o.rc == 0 and o.x is None and o.base is None and o.objrow is None and o.row_width is None
    same_state(first.state, keep)  # nothing was written to `in`
    same_own(o)
    assert o.status.tolist() == [w[3]["status"] for w in want]
    assert [tuple(p) for p in o.pivots.tolist()] == [w[3]["pivots"] for w in want]
    assert np.array_equal(bits(o.opt.cpu().numpy()), bits([w[3]["opt"] for w in want]))
    assert int(o.evicted.item()) == 0
    new = sx.BatchState.empty(B, n, m, "cuda")
    o = cut_call(n, m, B, dense(A0), dense(b0), dense(c), first.state, mask[0], cuts=q, state_out=new)
    assert o.rc == 0
    same_own(o)
    got = sx.BatchTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width, int(o.evicted.item()),
                          None, None, new)
    same_as_state_refs(got, [w[3] for w in want], n, m)
