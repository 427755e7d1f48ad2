"""A kept batch state grown by new constraint rows (simplex_solve_batch_device_rows), host side only
(no GPU): the entry's return codes, which are decided before any device is touched, the Python
wrapper's validation, and the specification itself checked on the oracle alone -- batch_rows_refs.py
restates the entry from batch_rhs_refs' dual loop, batch_state_refs._run and the oracle's fma, and the
GPU file compares the kernel with that restatement bit for bit, so what the restatement claims is
shown here:

  the grown state keeps the right-hand-side entry's identities, T[.][0] = S' b' and d[0] = y b'
  a warm start reaches the from-scratch solve's status on the grown problem and, up to the phase-1
  residue that a from-scratch solve keeps in its objective, its optimum
  a row that cuts the kept optimum off makes the dual loop pivot, a row that does not makes none
  a row no x >= 0 satisfies ends INFEASIBLE inside the dual loop
  a capped dual loop resumed is the uncapped one; a grown state takes a new right-hand side
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_rhs_refs import new_rhs, ref_rhs, ref_rhs_resume
from batch_rows_refs import (CAP_SHAPE, KINDS, ROWS_CAPS, THETAS, cuts_off, grow, grown_batch, lds_edge, ref_rows,
                             rows_shapes)
from batch_state_refs import bits, mixed_instances, ref_state, same_fields
from simplexoncuda_amd import _lib

# Rounding alone, relative to the optimum: the project's bound for a warm start that reaches the same
# vertex by another pivot path (test_batch_state_host.py, test_batch_rhs_host.py).
ROUNDING = 1e-10


# ------------------------------------------------------------------ return codes
def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host)"""
    base = dict(n=20, m=11, count=3, A=8, A_sb=220, A_sr=20, A_sc=1, b=8, b_sb=11, b_si=1, c=8, c_sb=20, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _call(args, sin=None, sout=None, added=1):
    lib = _lib.load()
    return lib.simplex_solve_batch_device_rows(None if args is None else ctypes.byref(args),
                                               None if sin is None else ctypes.byref(sin),
                                               None if sout is None else ctypes.byref(sout), added)


def test_rows_entry_argument_checks():
    """the right-hand-side entry's codes in its order, with A, b and c always read, `out` never `in`
    and `added` in [1, m); none needs a device"""
    assert _call(None) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=-1), _state()) == -1
    assert _call(_lib.BatchDeviceT(n=1, m=721, count=4), _state(), _state(2)) == -3  # a bad shape
    assert _call(_lib.BatchDeviceT(n=0, m=3, count=4), _state()) == -3
    # added out of range: no row, or no row left for the in-state
    for added in (0, -1, 11, 12):
        assert _call(_args(), _state(), _state(2), added) == -3, added
        assert _call(_lib.BatchDeviceT(n=20, m=11, count=0), _state(), _state(2), added) == -3, added
    assert _call(_args(), _state(), _state(2), 10) == -5
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=0), _state(), _state(2)) == 0
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=3), _state()) == -2  # every pointer null
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
    one = dict(n=1, m=2, count=1, A_sb=0, A_sc=0, b_sb=0, c_sb=0, c_sj=0)
    assert _call(_args(**one), _state(), None) == -5


def test_wrapper_validates_before_any_device_use():
    s = sx.BatchState.empty(3, 5, 4, torch.device("cpu"))
    f64 = dict(dtype=torch.float64)
    A, b, c = torch.ones((3, 6, 5), **f64), torch.ones((3, 6), **f64), torch.ones((3, 5), **f64)
    with pytest.raises(TypeError, match="must be a BatchState"):
        sx.add_rows_batch_tensors(None, A, b, c)
    with pytest.raises(TypeError, match="c must be a torch.Tensor"):
        sx.add_rows_batch_tensors(s, A, b, None)
    with pytest.raises(TypeError, match="float64"):
        sx.add_rows_batch_tensors(s, A, b.to(torch.float32), c)
    with pytest.raises(ValueError, match="c must be"):
        sx.add_rows_batch_tensors(s, A, b, c[:, :4])
    with pytest.raises(ValueError, match="state.T must be a contiguous"):
        sx.add_rows_batch_tensors(sx.BatchState(s.T[:, :3], s.d, s.base, s.phase, s.pivots, 5, 4), A, b, c)
    with pytest.raises(ValueError):
        sx.add_rows_batch_tensors(s, A, b[:, :5], c)
    with pytest.raises(ValueError, match="so b must be"):
        sx.add_rows_batch_tensors(s, A[:2], b[:2], c)
    # no appended row is not callable: added = 0, or fewer rows than the state has
    for m in (4, 3):
        with pytest.raises(ValueError, match="more rows than the state's 4"):
            sx.add_rows_batch_tensors(s, A[:, :m], b[:, :m], c)
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.add_rows_batch_tensors(s, A, b, c)


def test_shapes_the_gpu_file_relies_on():
    """the class of a launch is the grown shape's: (64, 63 -> 64) stays in the LDS class, (241, m0 -> m0
    + 1) leaves it, (241, 64 -> 65) is workspace to workspace; (4, 512 -> 513) puts the new row first
    in a second row tile, (600, 4 -> 5) has two tiles in the entering ratio; the in-state's dense
    stride 1 + n + m0 comes in both parities"""
    m0 = lds_edge(241)
    assert sx.batch_class(64, 63) == 2 and sx.batch_class(64, 64) == 2
    assert sx.batch_class(241, m0) == 2 and sx.batch_class(241, m0 + 1) == 1
    assert sx.batch_class(241, 64) == 1 and sx.batch_class(241, 65) == 1
    assert sx.batch_class(4, 512) == 1 and sx.batch_class(4, 513) == 1 and sx.batch_class(600, 5) == 2
    assert 513 > 512 and 600 + 5 > 512
    assert {(1 + n + m) % 2 for n, m, _ in rows_shapes()} == {0, 1}
    assert (5, 4, 3) in rows_shapes()


# ------------------------------------------------------------------ the restatement on the oracle
def _phase1_residue(A, b, c):
    """what a from-scratch solve's phase 1 leaves in d[0] (within eps of zero) and phase 2 keeps"""
    return abs(oracle.two_phase(A, b, c)["phase1_value"])


def _cases():
    """(shape, kind, theta, [(inst, grown)]) over every shape, kind of row and theta"""
    for n, m0, q in rows_shapes():
        for kind in KINDS:
            for theta in THETAS:
                yield (n, m0, q), kind, theta, list(zip(*grown_batch(n, m0, q, kind, theta)))


def test_identities():
    """on every grown state in phase 2: S' b' = T[:, 0] and y b' = d[0], S' the grown slack block and y
    the slack entries of the grown d (test_batch_rhs_host.py's test_identities on the grown state, new
    rows and their dual pivots included).  The column is compared relative to its largest entry; the
    kept objective still holds the in-state's phase-1 residue, so y b' is compared with it up to that
    residue.  Measured: 2.9e-14 for the column and 1.4e-15 for the objective (printed); the bounds
    leave a margin of 100 over them"""
    worst_col = worst_obj = 0.0
    pivoted = states = 0
    for _, _, _, pairs in _cases():
        for inst, (A, b, c) in pairs:
            st = ref_rows(ref_state(*inst), A, b, c)
            if st["phase"] != 2:
                continue
            states += 1
            pivoted += st["dual"] >= 1
            col, obj = new_rhs(st, b)
            worst_col = max(worst_col, np.abs(col - st["T"][:, 0]).max() / np.abs(st["T"][:, 0]).max())
            left = max(abs(obj - st["d"][0]) - _phase1_residue(*inst), 0.0)
            worst_obj = max(worst_obj, left / max(abs(st["d"][0]), 1.0))
    print(f"identities on the grown state: column {worst_col:.3e}, objective {worst_obj:.3e} relative")
    assert states >= 150 and pivoted >= 60
    assert worst_col <= 2.9e-12 and worst_obj <= 1.4e-13


def test_warm_start_against_scratch():
    """the same status as oracle.two_phase on the grown problem in every case, and the same optimum up
    to the from-scratch solve's phase-1 residue and rounding (prints the largest difference)"""
    worst = 0.0
    for shape, kind, theta, pairs in _cases():
        for inst, (A, b, c) in pairs:
            first = ref_state(*inst)
            warm = ref_rows(first, A, b, c)
            scratch = oracle.two_phase(A, b, c)
            assert warm["status"] == scratch["status"], (shape, kind, theta)
            assert warm["pivots"][0] == first["pivots"][0] and "dual" in warm
            assert warm["phase"] == (2 if warm["status"] == oracle.FEASIBLE else 3)
            if scratch["status"] == oracle.FEASIBLE:
                left = max(abs(warm["opt"] - scratch["opt"]) - abs(scratch["phase1_value"]), 0.0)
                worst = max(worst, left / abs(scratch["opt"]))
            else:
                assert np.isnan(warm["opt"]) and not bits(warm["x"]).any()
    print(f"warm added rows: largest relative objective difference beyond the phase-1 residue {worst:.3e}")
    assert worst <= ROUNDING


def test_dual_pivots_where_the_row_cuts():
    """a row that excludes the kept optimum -- a cut or a branch down at theta = 0.5, a branch up (-x_j
    <= -theta x*_j) at theta = 1.5 -- makes the dual loop pivot in every batch; a row that x* satisfies
    makes none: the cut and the branch down at theta = 1.5, the branch up at theta = 0.5.  One shape
    cannot pivot on a branch up: with n = 1 the only variable is basic in the only old row, the
    reduced new row has no negative entry and the loop ends INFEASIBLE at once"""
    for (n, m0, q), kind, theta, pairs in _cases():
        duals = [ref_rows(ref_state(*inst), *g)["dual"] for inst, g in pairs]
        if not cuts_off(kind, theta):
            assert duals == [0] * len(pairs), (n, m0, kind, theta)
        elif (n, kind) != (1, "up"):
            assert max(duals) >= 1, (n, m0, kind, theta)
        else:
            assert duals == [0] * len(pairs)


def test_impossible_row_is_infeasible_inside_the_dual_loop():
    for n, m0, q in rows_shapes():
        insts, grown = grown_batch(n, m0, q, "never", 0.5)
        for inst, (A, b, c) in zip(insts, grown):
            warm = ref_rows(ref_state(*inst), A, b, c)
            assert warm["status"] == oracle.INFEASIBLE and warm["phase"] == 3 and warm["pivots"][1] == warm["dual"]
            assert oracle.two_phase(A, b, c)["status"] == oracle.INFEASIBLE
            assert np.isnan(warm["opt"]) and not bits(warm["x"]).any()
            same_fields(ref_rhs_resume(warm, c), warm)  # again, without a pivot


def test_cold_start_is_two_phase_on_the_grown_problem():
    """phase-1 states and UNBOUNDED phase-2 states take the cold path: oracle.two_phase on the grown
    problem in every field"""
    row = np.ones(12)
    cold = 0
    for A0, b0, c in mixed_instances():
        st = ref_state(A0, b0, c)
        A, b = np.vstack([A0, row]), np.append(b0, 50.0)
        got = ref_rows(st, A, b, c)
        if "dual" in got:
            continue
        cold += 1
        assert (st["phase"], st["status"]) in ((1, oracle.INFEASIBLE), (2, oracle.UNBOUNDED))
        want = oracle.two_phase(A, b, c)
        want["row"] = oracle.last_objective_row().copy()
        same_fields(got, want, ("status", "pivots", "base", "row"))
    assert 0 < cold < len(mixed_instances())


def test_cap_then_resume_and_a_new_right_hand_side():
    n, m0, q = CAP_SHAPE
    insts, grown = grown_batch(n, m0, q, "cut", 0.5)
    most = 0
    for inst, (A, b, c) in zip(insts, grown):
        first = ref_state(*inst)
        whole = ref_rows(first, A, b, c)
        most = max(most, whole["dual"])
        for cap in [0] + ROWS_CAPS:
            capped = ref_rows(first, A, b, c, cap)
            if whole["pivots"][1] > cap:
                assert (capped["status"], capped["phase"], capped["pivots"][1]) == (oracle.PIVOT_CAP, 3, cap)
            same_fields(ref_rhs_resume(capped, c), whole)
        # the grown state takes a new right-hand side [m], and then another row
        again = ref_rhs(whole, A, 1.05 * b, c)
        assert again["status"] == oracle.two_phase(A, 1.05 * b, c)["status"]
        A3, b3, _ = grow((A, 1.05 * b, c), ["cut"], 0.5)
        third = ref_rows(again, A3, b3, c)
        assert third["status"] == oracle.two_phase(A3, b3, c)["status"] and third["T"].shape == (m0 + 2, 1 + n + m0 + 2)
    assert most >= 1
