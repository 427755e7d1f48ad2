"""The batched-solve kernels (sx_batch.hip k_batch_solve, k_batch_solve_dev) on tie-ladder LPs
(needs an MI355X).

wg_argmin is a second implementation of the eps-argmin tree: one workgroup walks the 512-wide
tiles one after the other, parks the tile winners and merges them with stage2_512.  On generated
instances no pivot depends on the combine order, so tests/test_gpu_batch*.py cannot tell a wrong
tree from the right one.  The whole LPs of tie_ladders.BATCH_CASES can: tests/test_tie_ladders.py
proves on the CPU that in every case the lane tree or the merge of the tile winners decides
pivots in both phases, and that a solver with np.argmin, or with the tile winners merged right to
left, returns something else than the oracle in a field compared here.

Bar: every field of both entries equals the oracle's, computed at test time, bit for bit
(batch_refs.same_as_refs) -- whole solves, and solves capped after k pivots of phase 1, which pin
the mid-solve objective row and basis.  A failure names the first pivot count at which the basis
differs (tie_ladders.explain_batch_divergence: bisection over the pivot cap, extra launches on a
failure only).

Also here, for the same kernels: compare()'s eligibility boundary as whole LPs, the lane-group
widths of the row update at their boundaries, and inner strides of b and c other than 1."""
import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
import tie_ladders as tl
from batch_refs import bits, ref_with_row, same_as_refs, same_tensors, tensors

pytestmark = pytest.mark.gpu

_INSTS = {}


def _stack(name):
    """the committed instance of a case and its neighbours of the next seeds (3 problems in the
    LDS class, 2 in the workspace class): built once, never written"""
    if name not in _INSTS:
        seed, cls = tl.BATCH_CASES[name][3], tl.BATCH_CASES[name][4]
        _INSTS[name] = [tl.make_batch(name, seed + k) for k in range(3 if cls == 2 else 2)]
    return _INSTS[name]


def _run_tensors(inst):
    def run(k):
        out = sx.solve_batch_tensors(*tensors([inst]), max_pivots=k)
        return int(out.status[0]), tuple(out.pivots[0].tolist()), out.base[0].cpu().numpy()
    return run


def _run_host(inst):
    def run(k):
        p = sx.Problem.from_arrays(*inst)
        try:
            r = sx.solve_batch([p], k)[0]
        finally:
            p.close()
        return r.status, tuple(r.pivots), r.base
    return run


def _explained(name, insts, run_of, compare):
    """compare(); when it fails, the failure with the first differing pivot count of every
    instance added"""
    try:
        compare()
    except AssertionError as err:
        why = ["problem %d: %s" % (k, tl.explain_batch_divergence(*inst, run_of(inst))) for k, inst in enumerate(insts)]
        pytest.fail("%s: %s\n%s" % (name, err, "\n".join(why)))


def _check_tensors(name, insts, max_pivots=-1):
    """one solve_batch_tensors call with the objective row against the oracle"""
    m, n = insts[0][0].shape
    out = sx.solve_batch_tensors(*tensors(insts), max_pivots=max_pivots, objective_row=True)
    refs = [ref_with_row(*abc, max_pivots=max_pivots) for abc in insts]
    _explained(name, insts, _run_tensors, lambda: same_as_refs(out, refs, n, m))
    return out, refs


def _same_as_ref_host(got, ref):
    """a solve_batch Result against the oracle's (the comparison of test_gpu_batch.py)"""
    assert got.status == ref["status"]
    assert tuple(got.pivots) == ref["pivots"]
    assert np.array_equal(got.base, ref["base"])
    if got.status == sx.FEASIBLE:
        assert np.array_equal(bits(got.optimal_value), bits(ref["opt"]))
        assert np.array_equal(bits(got.solution), bits(ref["x"]))


def _solve_host(insts, max_pivots=-1):
    probs = [sx.Problem.from_arrays(*abc) for abc in insts]
    try:
        return sx.solve_batch(probs, max_pivots)
    finally:
        for p in probs:
            p.close()


# ------------------------------------------------------------------ whole solves, device entry
@pytest.mark.parametrize("name", list(tl.BATCH_CASES))
def test_ladder_whole_solves_tensors(gpu, name):
    """the case and its seed neighbours in one call, in the class the case is sized for: every
    field and the final objective row.  (B-ws: 921 pivots of a 600 x 641 tableau in one workgroup)"""
    gen, (n, m, g), kw, seed, cls, pivots = tl.BATCH_CASES[name]
    assert sx.batch_class(n, m) == cls
    out, refs = _check_tensors(name, _stack(name))
    assert (refs[0]["status"], refs[0]["pivots"]) == (sx.FEASIBLE, pivots)
    assert out.evicted == 0
    assert max(max(r["pivots"]) for r in refs) <= 64 + 16 * (n + m)  # (the default resident budget covers them)


# ------------------------------------------------------------------ capped prefixes
def _caps(name):
    p1 = tl.BATCH_CASES[name][5][0]
    return sorted({k for k in (1, 2, 8, 40) if k < p1} | {p1})


_CAPPED = [(name, k) for name in tl.BATCH_CASES for k in _caps(name)]


@pytest.mark.parametrize("name,k", _CAPPED, ids=["%s-%d" % nk for nk in _CAPPED])
def test_ladder_capped_prefixes(gpu, name, k):
    """max_pivots = k inside phase 1 (k up to the oracle's phase-1 count, where the cap still comes
    before the phase's end is seen): PIVOT_CAP after exactly k pivots, and the full-width row d and
    the basis at that point -- the mid-solve state, where B-trim's divergence shows.  The seed
    neighbours ride along in the same call and end wherever the oracle says (a shorter phase 1 ends
    before the cap); the expectations spelled out below are the committed instance's"""
    n, m, _ = tl.BATCH_CASES[name][1]
    insts = _stack(name)
    inst = insts[0]
    out, refs = _check_tensors(name, insts, max_pivots=k)
    assert (refs[0]["status"], refs[0]["pivots"], len(refs[0]["row"])) == (sx.PIVOT_CAP, (k, 0), 1 + n + 2 * m)
    assert out.status[0].item() == sx.PIVOT_CAP and out.pivots[0].tolist() == [k, 0]
    assert out.row_width[0].item() == 1 + n + 2 * m and out.evicted == 0
    # the same state from k single pivots of the oracle on the phase-1 tableau
    T, d, base = tl.phase1_state(inst[0], inst[1])
    assert oracle.solve(T, d, base, max_pivots=k) == (oracle.PIVOT_CAP, k)
    assert np.array_equal(bits(out.objective_row[0].cpu().numpy()), bits(d))
    assert np.array_equal(out.base[0].cpu().numpy(), base)


def test_o_small_prefix_is_the_engine_case(gpu):
    """O-small after 40 pivots: the state test_gpu_tie_ladders.py holds every engine path to"""
    from test_gpu_tie_ladders import _case

    T0, d0, base0, k, (T, d, base) = _case("O-small")
    assert k == 40
    out = sx.solve_batch_tensors(*tensors([_stack("O-small")[0]]), max_pivots=k, objective_row=True)
    assert out.status.tolist() == [sx.PIVOT_CAP] and out.pivots.tolist() == [[k, 0]]
    assert np.array_equal(bits(out.objective_row[0].cpu().numpy()), bits(d))
    assert np.array_equal(out.base[0].cpu().numpy(), base)


# ------------------------------------------------------------------ whole solves, host entry
def test_ladder_whole_solves_host_entry(gpu):
    """all cases, ragged, in one solve_batch call: four in the LDS class, four in the workspace
    class, none on the engine"""
    names = list(tl.BATCH_CASES)
    insts = [_stack(name)[0] for name in names]
    refs = [ref_with_row(*abc) for abc in insts]
    got = _solve_host(insts)
    counts = sx.batch_counts()
    assert len(got) == len(insts)
    for name, inst, g, r in zip(names, insts, got, refs):
        assert (r["status"], r["pivots"]) == (sx.FEASIBLE, tl.BATCH_CASES[name][5])
        _explained(name, [inst], _run_host, lambda: _same_as_ref_host(g, r))
    cls = [tl.BATCH_CASES[name][4] for name in names]
    assert counts == (cls.count(2), cls.count(1), 0, 0) == (4, 4, 0, 0)


# ------------------------------------------------------------------ strided read, workspace class
def test_workspace_class_transposed_view(gpu):
    """B-ws through a transposed view of a [B, n, m] tensor: the build walks A by rows of the view's
    faster dimension (by_col == false) into a workspace slice"""
    n, m, _ = tl.BATCH_CASES["B-ws"][1]
    insts = _stack("B-ws")
    A, b, c = tensors(insts)
    want, _ = _check_tensors("B-ws", insts)
    At = A.transpose(1, 2).contiguous()
    keep = At.clone()
    view = At.transpose(1, 2)
    assert view.shape == A.shape and view.stride() == (n * m, 1, m)
    same_tensors(sx.solve_batch_tensors(view, b, c, objective_row=True), want)
    assert torch.equal(At, keep)


# ------------------------------------------------------------------ compare()'s eligibility boundary
_BOUNDARY_LPS = [(kind, where) for kind in ("entry", "cost") for where in ("below", "at", "above")]


def _boundary_insts():
    insts = [tl.boundary_lp(kind, tl.BOUNDARY[where]) for kind, where in _BOUNDARY_LPS]
    refs = [ref_with_row(*abc) for abc in insts]
    # (what tests/test_tie_ladders.py::test_boundary_lps_oracle asserts of the oracle)
    assert [(r["status"], r["pivots"]) for r in refs[:1] + refs[3:]] == [
        (sx.UNBOUNDED, (20, 0)), (sx.FEASIBLE, (20, 0)), (sx.FEASIBLE, (20, 1)), (sx.FEASIBLE, (20, 1))]
    assert all(r["pivots"][0] == 20 and r["pivots"][1] >= 1 for r in refs[1:3])
    return insts, refs


def test_eligibility_boundary_tensors(gpu):
    """an entering column whose largest entry, and a cost row whose only positive cost, is one ulp
    below 1e-9, 1e-9, one ulp above, as phase 2's first decision: `a >= SX_EPS` and
    cmp_eps(a, 0) > 0 in the ratio, cmp_eps(dmin, 0) < 0 in the phase's end"""
    insts, refs = _boundary_insts()
    assert sx.batch_class(6, 20) == 2
    out = sx.solve_batch_tensors(*tensors(insts), objective_row=True)
    same_as_refs(out, refs, 6, 20)
    assert out.evicted == 0


def test_eligibility_boundary_host_entry(gpu):
    insts, refs = _boundary_insts()
    for g, r in zip(_solve_host(insts), refs):
        _same_as_ref_host(g, r)
    assert sx.batch_counts() == (6, 0, 0, 0)


# ------------------------------------------------------------------ lane groups of the row update
# 1 + n + m = 16 | 17 and 32 | 33: the last widths with 16 and 32 lanes per row, the first with 32 and 64
_GROUP_SHAPES = [(8, 7), (9, 7), (20, 11), (20, 12)]


def _group_insts(n, m):
    return [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2, 3)]


@pytest.mark.parametrize("n,m", _GROUP_SHAPES)
def test_lane_group_boundaries_tensors(gpu, n, m):
    assert 1 + n + m in (16, 17, 32, 33)
    insts = _group_insts(n, m)
    out = sx.solve_batch_tensors(*tensors(insts), objective_row=True)
    refs = [ref_with_row(*abc) for abc in insts]
    assert all(r["pivots"][0] >= m for r in refs)  # (every row was updated, many times)
    same_as_refs(out, refs, n, m)
    assert out.evicted == 0


def test_lane_group_boundaries_host_entry(gpu):
    insts = [inst for n, m in _GROUP_SHAPES for inst in _group_insts(n, m)]
    for g, abc in zip(_solve_host(insts), insts):
        _same_as_ref_host(g, ref_with_row(*abc))
    assert sx.batch_counts() == (len(insts), 0, 0, 0)


# ------------------------------------------------------------------ inner strides of b and c
def test_inner_strides_of_b_and_c(gpu):
    """b as one column of a [B, m, 3] tensor (element stride 3), c as every second element of a
    [B, 2n] tensor (element stride 2): read in place, same tensors as the contiguous call"""
    n, m, _ = tl.BATCH_CASES["B-small"][1]
    insts = _stack("B-small")
    A, b, c = tensors(insts)
    B = len(insts)
    want, _ = _check_tensors("B-small", insts)
    b3 = torch.full((B, m, 3), -5.0, dtype=torch.float64, device="cuda")
    b3[:, :, 1] = b
    c2 = torch.full((B, 2 * n), 9.0, dtype=torch.float64, device="cuda")
    c2[:, ::2] = c
    keep = [t.clone() for t in (A, b3, c2)]
    bv, cv = b3[:, :, 1], c2[:, ::2]
    assert bv.stride() == (3 * m, 3) and cv.stride() == (2 * n, 2)
    same_tensors(sx.solve_batch_tensors(A, bv, cv, objective_row=True), want)
    assert all(torch.equal(t, k) for t, k in zip((A, b3, c2), keep))
