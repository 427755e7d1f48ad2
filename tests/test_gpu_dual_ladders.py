"""The kept-state batch entries (sx_batch.hip wg_dual, wg_drop, k_batch_solve_cut) on eps-ladder inputs
(needs an MI355X).

Six wg_argmin call sites arrived with the kept-state entries: the dual loop's entering ratio and leaving
row, the forced primal ratio with the slack moving up and on the negated column, the forced dual
entering ratio, and the Gomory source row.  On generated instances no selection of theirs depends on the
combine order of the eps-argmin tree, so a site that merged its tile winners linearly, or read a stale
mark, would pass every other test.  tests/dual_ladders.py builds inputs on which each site's pick is
decided by that order, and tests/test_dual_ladders.py proves on the CPU that the restatement with
np.argmin, or with the tile winners merged right to left, at that one site fails the comparison made here.

Bar: every field, the whole out-state and the objective row equal the restatement's (batch_rhs_refs,
batch_rows_refs, batch_drop_refs, batch_branch_refs, batch_cut_refs), computed at test time, bit for bit.
The committed case is problem 0 of its call and its seed neighbours ride along.  A failure says which
site's stand-in the device's result equals, if any (no extra launch)."""
import numpy as np
import pytest
import torch

import dual_ladders as dl
import oracle
import simplexoncuda_amd as sx
from batch_drop_refs import COLS, ROWS, reduced
from batch_refs import tensors
from batch_rhs_refs import ref_rhs, ref_rhs_resume, scaled_rhs
from batch_state_refs import bits, ref_state, same_as_state_refs

pytestmark = pytest.mark.gpu

_KEPT = {}


def _seeds(table, name):
    return [table[name][1] + k for k in range(dl.neighbours(table[name][2]))]


def _kept(key, insts):
    """one keep_state solve per set of instances in a session, checked against the reference: the state is
    never written (every call below leaves its in-state untouched)"""
    if key not in _KEPT:
        A, b, c = tensors(insts)
        out = sx.solve_batch_tensors(A, b, c, objective_row=True, keep_state=True)
        same_as_state_refs(out, [ref_state(*inst) for inst in insts], A.shape[2], A.shape[1])
        _KEPT[key] = (out.state, (A, b, c))
    return _KEPT[key]


def _dev(rows, dtype=np.float64):
    return torch.from_numpy(np.stack([np.asarray(r, dtype=dtype) for r in rows])).cuda()


def _rerhs(state, abc, b2s, **kw):
    return sx.resume_batch_tensors(state, abc[2], objective_row=True, A=abc[0], b=_dev(b2s), in_place=False, **kw)


def _held(check, wants, sites):
    """check(refs) compares the call's result with one restatement per problem.  When it fails for the true
    ones, the failure says which stand-in's restatement of problem 0 it passes with; sites: [(keyword,
    want(**selections) of problem 0)]"""
    true = [w() for w in wants]
    try:
        check(true)
    except AssertionError as err:
        hits = []
        for key, want in sites:
            for name, res in dl.standin_results(want, key).items():
                try:
                    check([res] + true[1:])
                    hits.append("%s with %s" % (key, name))
                except AssertionError:
                    pass
        pytest.fail("%s\nproblem 0 equals the restatement with: %s" % (err, ", ".join(hits) or "no stand-in"))
    return true


def _partial(f, *a, **k):
    from functools import partial
    return partial(f, *a, **k)


def _origin_batch(name):
    seeds = _seeds(dl.ORIGIN, name)
    cases = [dl.origin_case(name, s) for s in seeds]
    state, abc = _kept(("origin", name, tuple(seeds)), [(c["A"], c["b"], c["c"]) for c in cases])
    return cases, state, abc


# ------------------------------------------------------------------ the dual loop
@pytest.mark.parametrize("name", list(dl.ORIGIN))
def test_dual_loop_through_the_rhs_entry(gpu, name):
    """resume_batch_tensors(state, c, A=, b=b'): `groups` dual pivots, each with a leaving ladder over the
    ladder rows and an entering ladder d_j / 1.0 over the leaving row's group"""
    (n, m, _, _), _, cls, _, _ = dl.ORIGIN[name]
    assert sx.batch_class(n, m) == cls
    cases, state, abc = _origin_batch(name)
    out = _rerhs(state, abc, [c["b2"] for c in cases])
    assert out.evicted == 0
    want0 = _partial(dl.want_rhs, cases[0])
    _held(lambda refs: same_as_state_refs(out, refs, n, m), [_partial(dl.want_rhs, c) for c in cases],
          [("enter_argmin", want0), ("leave_argmin", want0)])


@pytest.mark.parametrize("name", [k for k, v in dl.ORIGIN.items() if v[3]])
def test_dual_loop_through_the_rows_entry(gpu, name):
    """the same entering ladder with the new row's slack leaving: the state of the instance without ladder
    row r_0, grown by the row -sum_{group 0} x_j <= -1"""
    (n, m, _, _), _, _, _, _ = dl.ORIGIN[name]
    rcs = [dl.rows_case(dl.origin_case(name, s)) for s in _seeds(dl.ORIGIN, name)]
    state, _ = _kept(("rows", name), [(r["A0"], r["b0"], r["c"]) for r in rcs])
    out = sx.add_rows_batch_tensors(state, *tensors([(r["A"], r["b"], r["c"]) for r in rcs]), objective_row=True)
    assert out.evicted == 0
    want0 = _partial(dl.want_rows, rcs[0])
    true = _held(lambda refs: same_as_state_refs(out, refs, n, m), [_partial(dl.want_rows, r) for r in rcs],
                 [("enter_argmin", want0)])
    assert true[0]["dual"] == 1


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("name", list(dl.ORIGIN))
def test_cap_inside_the_dual_loop_and_resume(gpu, name, cap):
    """max_pivots = 1 and 2: the phase-3 state after that many tree-decided pivots, tableau and all; its
    plain resume (rerhs = 0) is the uncapped re-solve"""
    (n, m, _, _), _, _, _, _ = dl.ORIGIN[name]
    cases, state, abc = _origin_batch(name)
    capped = _rerhs(state, abc, [c["b2"] for c in cases], max_pivots=cap)
    want0 = _partial(dl.want_rhs, cases[0], cap)
    crefs = _held(lambda refs: same_as_state_refs(capped, refs, n, m), [_partial(dl.want_rhs, c, cap) for c in cases],
                  [("enter_argmin", want0), ("leave_argmin", want0)])
    assert (crefs[0]["status"], crefs[0]["phase"], crefs[0]["pivots"][1]) == (sx.PIVOT_CAP, 3, cap)
    done = sx.resume_batch_tensors(capped.state, abc[2], objective_row=True, in_place=False)
    assert done.evicted == 0
    want0 = _partial(ref_rhs_resume, crefs[0], cases[0]["c"])
    whole = _held(lambda refs: same_as_state_refs(done, refs, n, m),
                  [_partial(ref_rhs_resume, r, c["c"]) for r, c in zip(crefs, cases)],
                  [("enter_argmin", want0), ("leave_argmin", want0)])
    assert dl.same_result(whole[0], dl.want_rhs(cases[0]))


# ------------------------------------------------------------------ the second step from K1
def _k1_batch(name):
    """the out-states K1 of a case and its neighbours, made on the GPU by the re-solve for b1 and held to
    the reference: (cases, BatchState)"""
    a = dl.SECOND[name][0]
    seeds = [dl.SECOND[name][1] + k for k in range(dl.neighbours(dl.ORIGIN[a][2]))]
    kcs = [dl.k1_case(dl.origin_case(a, s)) for s in seeds]
    key = ("k1", name)
    if key not in _KEPT:
        origins = [dl.origin_case(a, s) for s in seeds]
        state, abc = _kept(("origin", a, tuple(seeds)), [(c["A"], c["b"], c["c"]) for c in origins])
        out = _rerhs(state, abc, [k["b"] for k in kcs])
        m, n = kcs[0]["A"].shape
        same_as_state_refs(out, [k["state"] for k in kcs], n, m)
        _KEPT[key] = out.state
    return kcs, _KEPT[key]


def _drop_cols(state, kcs):
    small = [reduced((k["A"], k["b"], k["c"]), COLS, [k["e"]]) for k in kcs]
    out = sx.drop_cols_batch_tensors(state, _dev([[k["e"]] for k in kcs], np.int32), *tensors(small), objective_row=True)
    m, n = small[0][0].shape
    assert out.evicted == 0
    true = _held(lambda refs: same_as_state_refs(out, refs, n, m), [_partial(dl.want_drop_col, k) for k in kcs],
                 [("argmin", _partial(dl.want_drop_col, kcs[0]))])
    assert true[0]["path"] == "forced-dual"


@pytest.mark.parametrize("name", list(dl.SECOND))
def test_forced_dual_entering(gpu, name):
    """drop_cols_batch_tensors(K1, [e]): x_e is basic in row r_0, every candidate ratio d_j / 1.0 of the rest
    of its group lies within eps of every other, and its own column (ratio 0) is excluded"""
    kcs, state = _k1_batch(name)
    _drop_cols(state, kcs)


@pytest.mark.parametrize("name", list(dl.MINUS))
def test_forced_dual_entering_minus(gpu, name):
    """the same selection on a phase-3 state in which x_e's row has a negative right-hand side: the ladder
    stands on -lrow"""
    seeds = _seeds(dl.MINUS, name)
    mcs = [dl.minus_case(name, s) for s in seeds]
    state, abc = _kept(("minus", name), [(k["A"], k["b0"], k["c"]) for k in mcs])
    capped = _rerhs(state, abc, [k["b"] for k in mcs], max_pivots=1)
    m, n = mcs[0]["A"].shape
    same_as_state_refs(capped, [k["state"] for k in mcs], n, m)
    assert capped.state.phase.tolist() == [3] * len(mcs)
    _drop_cols(capped.state, mcs)


@pytest.mark.parametrize("name", list(dl.SECOND))
def test_branch_children(gpu, name):
    """x_e <= 0.5 and -x_e <= -1.5 as two children of every parent K1: the first reaches the dual loop's
    entering selection on K1's ladder through the branch front"""
    kcs, state = _k1_batch(name)
    m0, n = kcs[0]["A"].shape
    parent = [p for p in range(len(kcs)) for _ in dl.CHILDREN]
    child = [k for _ in kcs for k in range(len(dl.CHILDREN))]
    var = _dev([[kcs[p]["e"]] for p in parent], np.int32)
    coef, rhs = (_dev([[dl.CHILDREN[k][i]] for k in child]) for i in (0, 1))
    out = sx.branch_batch_tensors(state, _dev(parent, np.int32).reshape(-1), var, coef, rhs,
                                  *tensors([(k["A"], k["b"], k["c"]) for k in kcs]), objective_row=True)
    assert out.evicted == 0
    true = _held(lambda refs: same_as_state_refs(out, refs, n, m0 + 1),
                 [_partial(dl.want_child, kcs[p], k) for p, k in zip(parent, child)],
                 [("enter_argmin", _partial(dl.want_child, kcs[0], 0))])
    assert [t["dual"] for t in true[:2]] == [1, 1]


# ------------------------------------------------------------------ the forced primal ratio
def _drop_rows(name, q):
    ccs = [dl.chain_case(name, s, q) for s in _seeds(dl.CHAIN, name)]
    state, _ = _kept(("chain", name), [(c["A"], c["b"], c["c"]) for c in ccs])
    small = [reduced((c["A"], c["b"], c["c"]), ROWS, c["idx"]) for c in ccs]
    out = sx.drop_rows_batch_tensors(state, _dev([c["idx"] for c in ccs], np.int32), *tensors(small), objective_row=True)
    m, n = small[0][0].shape
    assert out.evicted == 0
    return _held(lambda refs: same_as_state_refs(out, refs, n, m), [_partial(dl.want_drop_rows, c) for c in ccs],
                 [("argmin", _partial(dl.want_drop_rows, ccs[0]))])


@pytest.mark.parametrize("name", list(dl.CHAIN))
def test_forced_primal_ratio(gpu, name):
    """drop_rows_batch_tensors of the row that bounds x_0 on the chain states: the dropped slack's column is
    +1.0 (forced+) or -1.0 (forced-) in every chain row and the ratios are the ladder x_i"""
    (L, m, sign), _, cls = dl.CHAIN[name]
    assert sx.batch_class(L + 1, m) == cls
    true = _drop_rows(name, 1)
    assert true[0]["paths"] == ["forced+" if sign > 0 else "forced-"]


def test_second_forced_ratio_on_the_shrunk_tableau(gpu):
    """q = 2 on the L = 24 chain: the row x_1 - x_0 <= . goes first, a tree-decided selection, and the
    second forced selection runs on the tableau the first one shrank"""
    true = _drop_rows("C+24", 2)
    assert true[0]["paths"] == ["forced+", "forced+"] and true[0]["forced"] == 2


# ------------------------------------------------------------------ the cut's source row
@pytest.mark.parametrize("cuts", [1, 3])
@pytest.mark.parametrize("name", list(dl.BOX))
def test_cut_source_rows(gpu, name, cuts):
    """cut_batch_tensors on the box states: all L box rows are eligible with the keys -(1/2 - q k_j); with
    three cuts the marks of the rows taken move the ladder between the selections"""
    (L, m0), _, cls = dl.BOX[name]
    n = L + 2
    assert sx.batch_class(n, m0 + 3) == cls
    xcs = [dl.box_case(name, s) for s in _seeds(dl.BOX, name)]
    state, (A0, b0, c) = _kept(("box", name), [(x["A"], x["b"], x["c"]) for x in xcs])
    B = len(xcs)
    A = torch.full((B, m0 + cuts, n), -7.0, dtype=torch.float64, device="cuda")
    b = torch.full((B, m0 + cuts), -7.0, dtype=torch.float64, device="cuda")
    A[:, :m0], b[:, :m0] = A0, b0
    out = sx.cut_batch_tensors(state, A, b, c, torch.ones(n, dtype=torch.bool, device="cuda"), cuts=cuts, objective_row=True)
    assert out.evicted == 0
    got_A, got_b, got_rows = A.cpu().numpy(), b.cpu().numpy(), out.cut_rows.cpu().numpy()

    def check(refs):
        for k, (cut_A, cut_b, cut_rows, _) in enumerate(refs):
            assert np.array_equal(got_rows[k], cut_rows), (k, got_rows[k], cut_rows)
            assert np.array_equal(bits(got_A[k, m0:]), bits(cut_A)) and np.array_equal(bits(got_b[k, m0:]), bits(cut_b)), k
        same_as_state_refs(out, [r[3] for r in refs], n, m0 + cuts)

    true = _held(check, [_partial(dl.want_cut, x, cuts) for x in xcs], [("argmin", _partial(dl.want_cut, xcs[0], cuts))])
    # the tree's successive picks (tests/test_dual_ladders.py::test_box_state derives them from the keys)
    assert got_rows[0].tolist() == dl.want_cut(xcs[0], 3)[2][:cuts].tolist()


# ------------------------------------------------------------------ batch position
def test_batch_position(gpu):
    """A-1t between two generated instances of its shape, first and last in the call: the same bits"""
    name = "A-1t"
    (n, m, _, _), _, _, _, _ = dl.ORIGIN[name]
    case = dl.origin_case(name)
    lad = ((case["A"], case["b"], case["c"]), case["b2"])
    gen = [(inst, scaled_rhs(inst[1], 77 + k, 1.0)) for k, inst in
           enumerate(oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2))]
    outs = []
    for pos, batch in ((0, [lad] + gen), (2, gen + [lad])):
        insts = [inst for inst, _ in batch]
        state, abc = _kept(("position", pos), insts)
        out = _rerhs(state, abc, [b2 for _, b2 in batch])
        refs = [ref_rhs(ref_state(*inst), inst[0], b2, inst[2]) for inst, b2 in batch]
        assert refs[pos]["dual"] >= 4 and any(r.get("dual", 0) >= 1 for k, r in enumerate(refs) if k != pos)
        same_as_state_refs(out, refs, n, m)
        outs.append((out, pos))
    (x, i), (y, j) = outs
    for f in ("status", "pivots", "base", "row_width"):
        assert torch.equal(getattr(x, f)[i], getattr(y, f)[j]), f
    for f in ("optimal_value", "solution", "objective_row"):
        assert torch.equal(getattr(x, f)[i].view(torch.int64), getattr(y, f)[j].view(torch.int64)), f
    for f in ("T", "d"):
        assert torch.equal(getattr(x.state, f)[i].view(torch.int64), getattr(y.state, f)[j].view(torch.int64)), f
