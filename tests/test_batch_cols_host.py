"""A kept batch state grown by new structural columns (simplex_solve_batch_device_cols), host side only
(no GPU): the entry's return codes, which are decided before any device is touched, the Python
wrapper's validation, and the specification itself checked on the oracle alone -- batch_cols_refs.py
restates the entry from batch_rhs_refs' sums and dual loop, batch_state_refs._run and the oracle's
gemv_partials, and the GPU file compares the kernel with that restatement bit for bit, so what the
restatement claims is shown here:

  a new stored column is B^-1 D a and its reduced cost c_B^T B^-1 D a - c_new for the grown basis matrix
  a warm start reaches the from-scratch solve's status on the grown problem and its optimum
  a column that does not price in makes no pivot, one that does makes phase 2 pivot, a non-positive
  column with a positive cost ends UNBOUNDED
  an elastic column rescues a state that stands INFEASIBLE inside the dual loop
  a capped warm phase 2 resumed is the uncapped one; rows, a new right-hand side and further columns
  follow on a grown state
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_cols_refs import (CAP_SHAPE, COLS_CAPS, KINDS, RESCUE_SHAPES, append_column, cols_shapes, elastic, lds_edge,
                             many_grown, kept_part, ref_cols, want_batch)
from batch_rhs_refs import negated_rhs, new_rhs, ref_rhs, ref_rhs_resume
from batch_rows_refs import grow, ref_rows
from batch_state_refs import _negative, bits, mixed_instances, ref_state, same_fields, save_instances
from simplexoncuda_amd import _lib

# Rounding alone, relative to the optimum: the project's bound for a warm start that reaches the same
# vertex by another pivot path (test_batch_state_host.py, test_batch_rhs_host.py, test_batch_rows_host.py).
ROUNDING = 1e-10


# ------------------------------------------------------------------ return codes
def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host)"""
    base = dict(n=21, m=10, count=3, A=8, A_sb=210, A_sr=21, A_sc=1, b=8, b_sb=10, b_si=1, c=8, c_sb=21, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _call(args, sin=None, sout=None, added=1):
    lib = _lib.load()
    return lib.simplex_solve_batch_device_cols(None if args is None else ctypes.byref(args),
                                               None if sin is None else ctypes.byref(sin),
                                               None if sout is None else ctypes.byref(sout), added)


def test_cols_entry_argument_checks():
    """the rows entry's codes in its order, with A, b and c always read, `out` never `in` and `added`
    in [1, n); none needs a device"""
    assert _call(None) == -1
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=-1), _state()) == -1
    assert _call(_lib.BatchDeviceT(n=2, m=721, count=4), _state(), _state(2)) == -3  # a grown shape of class 0
    assert sx.batch_class(2, 721) == 0
    assert _call(_lib.BatchDeviceT(n=3, m=0, count=4), _state()) == -3
    # added out of range: no column, or no column left for the in-state
    for added in (0, -1, 21, 22):
        assert _call(_args(), _state(), _state(2), added) == -3, added
        assert _call(_lib.BatchDeviceT(n=21, m=10, count=0), _state(), _state(2), added) == -3, added
    assert _call(_args(), _state(), _state(2), 20) == -5
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=0), _state(), _state(2)) == 0
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=3), _state()) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), _state(), _state(2)) == -2, f
    # `in` is required
    assert _call(_args(), None, _state(2)) == -2
    assert _call(_args(), None, None) == -2
    # a NULL member of a state struct that is passed
    for f in ("T", "d", "base", "phase", "pivots"):
        bad = _state()
        setattr(bad, f, None)
        assert _call(_args(), bad, _state(2)) == -2, f
        assert _call(_args(), bad, None) == -2, f
        bad = _state(2)
        setattr(bad, f, None)
        assert _call(_args(), _state(), bad) == -2, f
    # `out` shares a member with `in`: the shapes differ, so in place is impossible
    assert _call(_args(), _state(), _state()) == -2
    for f in ("T", "d", "base", "phase", "pivots"):
        shared = _state(2)
        setattr(shared, f, 1)
        assert _call(_args(), _state(), shared) == -2, f
    # A, b and c are required and every stride is checked
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), _state(), _state(2)) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), _state(), _state(2)) == -4, f
    # ... and then every check up to the workspace's is passed
    assert _call(_args(), _state(), _state(2)) == -5
    assert _call(_args(), _state(), None) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20), _state(), None) == -5   # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255), _state(), None) == -5    # no header
    # a stride of 0 along a dimension of length 1 is accepted, as in the device entry
    one = dict(n=2, m=1, count=1, A_sb=0, A_sr=0, b_sb=0, b_si=0, c_sb=0)
    assert _call(_args(**one), _state(), None) == -5


def test_wrapper_validates_before_any_device_use():
    s = sx.BatchState.empty(3, 5, 4, torch.device("cpu"))
    f64 = dict(dtype=torch.float64)
    A, b, c = torch.ones((3, 4, 6), **f64), torch.ones((3, 4), **f64), torch.ones((3, 6), **f64)
    with pytest.raises(TypeError, match="must be a BatchState"):
        sx.add_cols_batch_tensors(None, A, b, c)
    with pytest.raises(TypeError, match="c must be a torch.Tensor"):
        sx.add_cols_batch_tensors(s, A, b, None)
    with pytest.raises(TypeError, match="float64"):
        sx.add_cols_batch_tensors(s, A, b.to(torch.float32), c)
    with pytest.raises(TypeError, match="float64"):
        sx.add_cols_batch_tensors(s, A, b, c.to(torch.float32))
    with pytest.raises(ValueError, match="c must be"):
        sx.add_cols_batch_tensors(s, A, b, c[0])
    with pytest.raises(ValueError, match="c must be"):
        sx.add_cols_batch_tensors(s, A, b, c[:2])
    with pytest.raises(ValueError, match="state.T must be a contiguous"):
        sx.add_cols_batch_tensors(sx.BatchState(s.T[:, :3], s.d, s.base, s.phase, s.pivots, 5, 4), A, b, c)
    with pytest.raises(ValueError, match="so b must be"):
        sx.add_cols_batch_tensors(s, A, b[:, :3], c)
    with pytest.raises(ValueError, match="so b must be"):
        sx.add_cols_batch_tensors(s, A, b, c[:, :5])
    # no appended column is not callable: added = 0, or fewer columns than the state has
    for n in (5, 4):
        with pytest.raises(ValueError, match="more columns than the state's 5"):
            sx.add_cols_batch_tensors(s, A[:, :, :n], b, c[:, :n])
    # the rows are the state's
    with pytest.raises(ValueError, match=r"A must be \[3, 4, n\]"):
        sx.add_cols_batch_tensors(s, torch.ones((3, 5, 6), **f64), torch.ones((3, 5), **f64), c)
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.add_cols_batch_tensors(s, A, b, c)


def test_shapes_the_gpu_file_relies_on():
    """the class of a launch is the grown shape's: (63 -> 64, 64) stays in the LDS class, (240 -> 241, 64)
    leaves it (240 is the edge batch_class gives at m = 64), (241 -> 242, 64) is workspace to workspace;
    (4 -> 5, 513) has two row tiles in the leaving ratio; the new column of (511 -> 512, 4) is candidate
    511 of the entering selection, the last of its first tile, that of (512 -> 513, 4) candidate 512, the
    first of the second tile; (599 -> 600, 4) selects over two tiles; the in-state's dense stride
    1 + n0 + m comes in both parities"""
    assert lds_edge(64) == 240
    assert sx.batch_class(63, 64) == 2 and sx.batch_class(64, 64) == 2
    assert sx.batch_class(240, 64) == 2 and sx.batch_class(241, 64) == 1 and sx.batch_class(242, 64) == 1
    assert sx.batch_class(4, 513) == 1 and sx.batch_class(5, 513) == 1
    assert sx.batch_class(512, 4) == 2 and sx.batch_class(513, 4) == 2 and sx.batch_class(600, 4) == 2
    shapes = cols_shapes()
    assert len(shapes) == 12 and len(set(shapes)) == 12
    assert {(1 + n0 + m) % 2 for n0, _, m in shapes} == {0, 1}
    assert (5, 3, 4) in shapes and (240, 1, 64) in shapes and (241, 1, 64) in shapes
    # the entering selection runs over d[1 .. Ns): a variable's candidate index is its own index
    assert 1 + 599 + 4 - 1 > 512


# ------------------------------------------------------------------ the restatement on the oracle
def _cases():
    """(shape, kind, theta, kept, grown, refs, want) over every shape and kind of column"""
    for shape in cols_shapes():
        for kind, theta in KINDS:
            yield (shape, kind, theta) + want_batch(*shape, kind, theta)


def test_which_instances_pivot():
    """theta = 0.01: no warm pivot in any instance; theta = 100: at least one instance of every batch
    pivots; the negated column: UNBOUNDED warm and from scratch in every instance.  No case is cold"""
    for shape, kind, theta, _, grown, refs, want in _cases():
        assert all(r["status"] == oracle.FEASIBLE and r["phase"] == 2 for r in refs), shape
        assert not any(w["cold"] for w in want)
        assert all(w["pivots"][0] == r["pivots"][0] and w["phase"] == 2 for w, r in zip(want, refs))
        warm = [w["pivots"][1] for w in want]
        if kind == "unbounded":
            assert all(w["status"] == oracle.UNBOUNDED for w in want), shape
            assert all(oracle.two_phase(*g)["status"] == oracle.UNBOUNDED for g in grown), shape
        elif theta < 1.0:
            assert warm == [0] * len(want), (shape, warm)
        else:
            assert max(warm) >= 1, (shape, warm)


def _basis(A, b, base):
    """the basis matrix of [D A | D] for the basis `base`, D, and the basic costs' selector"""
    m, n = A.shape
    D = np.diag([-1.0 if _negative(x) else 1.0 for x in b])
    full = np.hstack([D @ A, D])
    return full[:, base], D


def test_identities():
    """on every grown phase-2 state: the stored column of a new variable is B^-1 D a and its entry of d
    is c_B^T B^-1 D a - c_new, B the grown state's own basis matrix (a direct solve, numpy's LU); the
    column relative to its largest entry, the reduced cost relative to the larger of 1 and the sum of
    the magnitudes it is made of.  Measured: 2.3e-10 for the column and 2.2e-12 for the reduced cost
    (printed), both on a (240 -> 241, 64) state that ended UNBOUNDED behind 108 warm pivots with a basis
    of condition 4e7, where the old columns deviate as much (7.5e-11); the states that end FEASIBLE stay
    below 1e-13.  The bounds leave a margin of 100 over the measured figures"""
    worst_col = worst_red = 0.0
    states = pivoted = 0
    where = {}
    for (n0, p, m), kind, theta, _, grown, refs, want in _cases():
        for (A, b, c), st in zip(grown, want):
            if st["phase"] != 2 or st["status"] == oracle.PIVOT_CAP:
                continue
            states += 1
            pivoted += st["pivots"][1] >= 1
            B, D = _basis(A, b, st["base"])
            cB = np.array([c[j] if j < n0 + p else 0.0 for j in st["base"]])
            for t in range(p):
                col = np.linalg.solve(B, D @ A[:, n0 + t])
                got = st["T"][:, 1 + n0 + t]
                dev_col = np.abs(col - got).max() / np.abs(col).max()
                red = cB @ col - c[n0 + t]
                scale = max(np.abs(cB * col).sum() + abs(c[n0 + t]), 1.0)
                dev_red = abs(red - st["d"][1 + n0 + t]) / scale
                if dev_col > worst_col:
                    worst_col, where["column"] = dev_col, (n0, p, m)
                if dev_red > worst_red:
                    worst_red, where["reduced cost"] = dev_red, (n0, p, m)
    print(f"identities on the grown state, {states} states: column {worst_col:.3e}, reduced cost {worst_red:.3e} "
          f"relative, at {where}")
    assert states >= 100 and pivoted >= 25
    assert worst_col <= 2.3e-8 and worst_red <= 2.2e-10


def test_slack_block_identities_survive():
    """S is unchanged by the load, so the right-hand-side entry's identities T[:, 0] = S b and d[0] = y b
    hold on the grown state as they did on the kept one (test_batch_rhs_host.py's bounds)"""
    for (n0, p, m), kind, theta, _, grown, refs, want in _cases():
        if kind != "scaled" or theta < 1.0 or m > 64:
            continue
        for (A, b, c), st in zip(grown, want):
            col, obj = new_rhs(st, b)
            assert np.abs(col - st["T"][:, 0]).max() <= 1e-9 * max(np.abs(st["T"][:, 0]).max(), 1.0)
            residue = abs(oracle.two_phase(*kept_part((A, b, c), n0))["phase1_value"])
            assert max(abs(obj - st["d"][0]) - residue, 0.0) <= 1e-9 * max(abs(st["d"][0]), 1.0)


def test_warm_start_against_scratch():
    """the same status as oracle.two_phase on the grown problem in every case, and the same optimum to
    the project's bound for two pivot paths to one vertex.  A from-scratch solve keeps its phase-1
    residue in d[0]; the warm start keeps the kept state's.  Measured (printed): 4.2e-12 relative as
    it stands, at (4 -> 5, 513), and 2.0e-15 with the two residues set aside"""
    worst = worst_left = 0.0
    cases = 0
    for (n0, p, m), kind, theta, kept, grown, refs, want in _cases():
        for k0, (A, b, c), warm in zip(kept, grown, want):
            cases += 1
            scratch = oracle.two_phase(A, b, c)
            assert warm["status"] == scratch["status"], ((n0, p, m), kind, theta)
            if scratch["status"] == oracle.FEASIBLE:
                diff = abs(warm["opt"] - scratch["opt"])
                residue = abs(scratch["phase1_value"]) + abs(oracle.two_phase(*k0)["phase1_value"])
                worst = max(worst, diff / abs(scratch["opt"]))
                worst_left = max(worst_left, max(diff - residue, 0.0) / abs(scratch["opt"]))
            else:
                assert np.isnan(warm["opt"]) and not bits(warm["x"]).any()
    print(f"warm added columns, {cases} cases: largest relative objective difference {worst:.3e}, "
          f"{worst_left:.3e} beyond the phase-1 residues")
    assert cases == 108
    assert worst <= ROUNDING


def test_elastic_column_rescues_a_phase_3_state():
    """states left INFEASIBLE inside the dual loop by b_0 negated: the elastic column -e_0 with cost
    -1000 is warm, one dual pivot, FEASIBLE, and the from-scratch solve agrees; with cost +1 the grown
    row is not dual feasible and the problem is cold"""
    for n, m in RESCUE_SHAPES:
        for A, b, c in save_instances(n, m):
            b2 = negated_rhs(b, 0)
            stuck = ref_rhs(ref_state(A, b, c), A, b2, c)
            assert stuck["status"] == oracle.INFEASIBLE and stuck["phase"] == 3
            g = elastic((A, b2, c), -1000.0)
            warm = ref_cols(stuck, *g)
            assert not warm["cold"] and warm["dual"] == 1 and warm["status"] == oracle.FEASIBLE and warm["phase"] == 2
            assert warm["pivots"][0] == stuck["pivots"][0]
            scratch = oracle.two_phase(*g)
            assert scratch["status"] == oracle.FEASIBLE
            assert abs(warm["opt"] - scratch["opt"]) <= ROUNDING * abs(scratch["opt"])
            g = elastic((A, b2, c), 1.0)
            cold = ref_cols(stuck, *g)
            assert cold["cold"]
            same_fields(cold, ref_state(*g))


def test_cold_start_is_two_phase_on_the_grown_problem():
    """the mixed batch: phase-1 states take the cold path, oracle.two_phase on the grown problem in
    every field; UNBOUNDED and FEASIBLE phase-2 states are warm and reach its status"""
    cold = 0
    kinds = set()
    for A0, b0, c0 in mixed_instances():
        st = ref_state(A0, b0, c0)
        kinds.add((st["phase"], st["status"]))
        A, b, c = np.hstack([A0, np.ones((len(b0), 1))]), b0, np.append(c0, 50.0)
        got = ref_cols(st, A, b, c)
        want = oracle.two_phase(A, b, c)
        assert got["status"] == want["status"]
        assert got["cold"] == (st["phase"] == 1)
        if got["cold"]:
            cold += 1
            want["row"] = oracle.last_objective_row().copy()
            same_fields(got, want, ("status", "pivots", "base", "row"))
    assert kinds >= {(1, oracle.INFEASIBLE), (2, oracle.UNBOUNDED), (2, oracle.FEASIBLE)}
    assert 0 < cold < len(mixed_instances())


def test_cap_then_resume_and_what_follows():
    n0, p, m = CAP_SHAPE
    _, grown, refs, whole = want_batch(n0, p, m, "scaled", 100.0)
    assert sorted(w["pivots"][1] for w in whole)[1] > max(COLS_CAPS)
    for first, (A, b, c), w in zip(refs, grown, whole):
        for cap in [0] + COLS_CAPS:
            capped = ref_cols(first, A, b, c, cap)
            if w["pivots"][1] > cap:
                assert (capped["status"], capped["phase"], capped["pivots"][1]) == (oracle.PIVOT_CAP, 2, cap)
            same_fields(ref_rhs_resume(capped, c), w)
        # the grown state takes a row, a new right-hand side [m] and another column
        A2, b2, c2 = grow((A, b, c), ["cut"], 0.5)
        second = ref_rows(w, A2, b2, c2)
        assert second["status"] == oracle.two_phase(A2, b2, c2)["status"]
        third = ref_rhs(second, A2, 1.05 * b2, c2)
        assert third["status"] == oracle.two_phase(A2, 1.05 * b2, c2)["status"]
        g4 = append_column((A2, 1.05 * b2, c2), 900, 100.0)
        fourth = ref_cols(third, *g4)
        assert fourth["status"] == oracle.two_phase(*g4)["status"] and fourth["T"].shape == (m + 1, 1 + n0 + 2 + m + 1)


def test_many_problems_pivot():
    warm = 0
    for g in many_grown()[::12]:
        w = ref_cols(ref_state(*kept_part(g, 5)), *g)
        assert not w["cold"] and w["status"] == oracle.two_phase(*g)["status"]
        warm += w["pivots"][1] >= 1
    assert warm >= 10
