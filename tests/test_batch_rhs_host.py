"""A kept batch state re-solved for a new right-hand side (simplex_solve_batch_device_rhs), host
side only (no GPU): the entry's return codes, which are decided before any device is touched, the
Python wrapper's validation, and the specification itself checked on the oracle alone --
batch_rhs_refs.py restates the entry from the oracle's argmin, ratio, gemv_partials and apply_update
and batch_state_refs._run, and the GPU file compares the kernel with that restatement bit for bit, so
what the restatement claims is shown here:

  its cold start is oracle.two_phase in every field
  S b and y b on the unchanged b reproduce the kept right-hand-side column and objective
  a warm re-solve reaches the from-scratch solve's status and, up to the phase-1 residue that a
  from-scratch solve keeps in its objective, its optimum, in no more pivots than that solve took
  a right-hand side with one entry negated ends INFEASIBLE both ways
  a capped dual loop resumed is the uncapped one; a finished state ends again without a pivot
  the leaving row depends on the eps-argmin's combine order on the ladder cases
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_rhs_refs import (HOST_SCALES, PHASE2_CAP, PHASE2_CAP_SHAPE, RHS_CAPS, RHS_SHAPES, dual_feasible, first_min,
                            ladder_cases, negated_rhs, new_rhs, ref_rhs, ref_rhs_resume, rhs_instances, scaled_batch)
from batch_state_refs import WARM_SHAPES, bits, mixed_instances, ref_state, same_fields, warm_instances
from simplexoncuda_amd import _lib

# Rounding alone, relative to the optimum: test_batch_state_host.py's bound for a warm start that reaches
# the same vertex by another pivot path.
ROUNDING = 1e-10


# ------------------------------------------------------------------ return codes
def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host)"""
    base = dict(n=20, m=10, count=3, A=8, A_sb=200, A_sr=20, A_sc=1, b=8, b_sb=10, b_si=1, c=8, c_sb=20, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _call(args, sin=None, sout=None, rerhs=0):
    lib = _lib.load()
    return lib.simplex_solve_batch_device_rhs(None if args is None else ctypes.byref(args),
                                              None if sin is None else ctypes.byref(sin),
                                              None if sout is None else ctypes.byref(sout), rerhs)


def test_rhs_entry_argument_checks():
    """the state entry's codes in its order, with `in` required and A, b read only with rerhs; none
    needs a device"""
    assert _call(None) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=-1), _state()) == -1
    assert _call(_lib.BatchDeviceT(n=1, m=721, count=4), _state(), _state(), 1) == -3  # a bad shape
    assert _call(_lib.BatchDeviceT(n=0, m=3, count=4), _state()) == -3
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=0), _state(), _state(), 1) == 0
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=3), _state()) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), _state(), _state(), 1) == -2, f
    # `in` is required, with or without rerhs
    assert _call(_args(), None, _state(), 0) == -2
    assert _call(_args(), None, _state(), 1) == -2
    assert _call(_args(), None, None, 1) == -2
    # a NULL member of a state struct that is passed
    for f in ("T", "d", "base", "phase", "pivots"):
        bad = _state()
        setattr(bad, f, None)
        assert _call(_args(), bad, _state(), 1) == -2, f
        assert _call(_args(), _state(), bad, 1) == -2, f
        assert _call(_args(), bad, None, 0) == -2, f
    # with rerhs A, b and c are required and every stride is checked
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), _state(), _state(), 1) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), _state(), _state(), 1) == -4, f
    # without it only c is read: A and b may be NULL with any strides, c may not
    resume = dict(A=None, b=None, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0)
    assert _call(_args(c=None, **resume), _state(), _state(), 0) == -2
    for f in ("c_sb", "c_sj"):
        assert _call(_args(**{f: 0}, **resume), _state(), None, 0) == -4, f
    assert _call(_args(**resume), _state(), _state(), 1) == -2
    # ... and then every check up to the workspace's is passed
    assert _call(_args(**resume), _state(), _state(), 0) == -5
    assert _call(_args(), _state(), _state(), 1) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20), _state(), None, 1) == -5      # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255), _state(), None, 1) == -5       # no header
    assert _call(_args(workspace=4096, workspace_bytes=255, **resume), _state(), None, 0) == -5
    # a stride of 0 along a dimension of length 1 is accepted, as in the device entry
    one = dict(n=1, m=1, count=1, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0, c_sb=0, c_sj=0)
    assert _call(_args(**one), _state(), None, 1) == -5


def test_wrapper_validates_before_any_device_use():
    s = sx.BatchState.empty(3, 5, 4, torch.device("cpu"))
    assert s.rhs is False
    A, b, c = torch.ones((3, 4, 5), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float64), \
        torch.ones((3, 5), dtype=torch.float64)
    with pytest.raises(ValueError, match="needs A and b, both"):
        sx.resume_batch_tensors(s, c, A=A)
    with pytest.raises(ValueError, match="needs A and b, both"):
        sx.resume_batch_tensors(s, c, b=b)
    with pytest.raises(ValueError, match="recost is not combined"):
        sx.resume_batch_tensors(s, c, recost=True, A=A, b=b)
    with pytest.raises(ValueError, match="needs A and b, both"):
        sx.resume_batch_tensors(s, c, recost=True, b=b)
    with pytest.raises(ValueError):
        sx.resume_batch_tensors(s, c, A=A[:, :3], b=b)
    with pytest.raises(TypeError, match="float64"):
        sx.resume_batch_tensors(s, c, A=A, b=b.to(torch.float32))
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.resume_batch_tensors(s, c, A=A, b=b)


def test_shapes_the_gpu_file_relies_on():
    """(241, 64) is a workspace-class shape, (4, 513) has two row tiles in the leaving argmin and
    (600, 4) two tiles in the entering ratio"""
    assert sx.batch_class(241, 64) == 1 and sx.batch_class(4, 513) == 1 and sx.batch_class(600, 4) == 2
    assert 513 > 512 and 600 + 4 > 512


# ------------------------------------------------------------------ the restatement on the oracle
def test_cold_start_is_two_phase():
    """phase-1 states, UNBOUNDED phase-2 states and a state capped in phase 2 take the cold path,
    which is oracle.two_phase on the new right-hand side in every field"""
    cold = capped2 = 0
    for insts, caps in ((mixed_instances(), (-1, 15)), (rhs_instances(*PHASE2_CAP_SHAPE), (PHASE2_CAP,))):
        for (A, b, c), b2 in zip(insts, scaled_batch(insts, 0.1)):
            for cap in caps:
                st = ref_state(A, b, c, cap)
                if st["phase"] != 1 and dual_feasible(st):
                    continue
                cold += 1
                capped2 += st["phase"] == 2 and st["status"] == oracle.PIVOT_CAP
                want = oracle.two_phase(A, b2, c)
                want["row"] = oracle.last_objective_row().copy()
                got = ref_rhs(st, A, b2, c)
                same_fields(got, want, ("status", "pivots", "base", "row"))
                if want["status"] == oracle.FEASIBLE:
                    same_fields(got, want, ("opt", "x"))
                else:
                    assert np.isnan(got["opt"]) and not bits(got["x"]).any()
    states = [ref_state(*inst) for inst in mixed_instances()]
    assert {(s["phase"], s["status"]) for s in states} >= {(1, oracle.INFEASIBLE), (2, oracle.UNBOUNDED),
                                                           (2, oracle.FEASIBLE)}
    assert cold >= 30 and capped2 == 3


def _phase1_residue(A, b, c):
    """what a from-scratch solve's phase 1 leaves in d[0] (within eps of zero) and phase 2 keeps"""
    return abs(oracle.two_phase(A, b, c)["phase1_value"])


def test_identities():
    """S b = T[:, 0] and y b = d[0] on the unchanged b, negated rows included.  The column is compared
    relative to its largest entry.  The kept objective still holds phase 1's residue, so y b is
    compared with it up to that residue.  Measured: 4.9e-15 for the column and 2.1e-14 for the
    objective (printed); the bounds leave a margin of 100 over them"""
    worst_col = worst_obj = 0.0
    negated = 0
    sets = [rhs_instances(n, m) for n, m in RHS_SHAPES] + [warm_instances(n, m) for n, m in WARM_SHAPES]
    for insts in sets + [mixed_instances()]:
        for A, b, c in insts:
            st = ref_state(A, b, c)
            if st["phase"] != 2:
                continue
            negated += (b < 0).any()
            col, obj = new_rhs(st, b)
            worst_col = max(worst_col, np.abs(col - st["T"][:, 0]).max() / np.abs(st["T"][:, 0]).max())
            left = max(abs(obj - st["d"][0]) - _phase1_residue(A, b, c), 0.0)
            worst_obj = max(worst_obj, left / max(abs(st["d"][0]), 1.0))
    print(f"identities: column {worst_col:.3e}, objective {worst_obj:.3e} relative")
    assert negated >= 10
    assert worst_col <= 4.9e-13 and worst_obj <= 2.1e-12


def _against_scratch(insts, scale):
    """(largest relative objective difference beyond the residue, most warm pivots) of one batch"""
    worst, most = 0.0, 0
    for (A, b, c), b2 in zip(insts, scaled_batch(insts, scale)):
        first = ref_state(A, b, c)
        assert first["status"] == oracle.FEASIBLE and first["phase"] == 2 and dual_feasible(first)
        scratch = ref_state(A, b2, c)
        warm = ref_rhs(first, A, b2, c)
        assert warm["status"] == scratch["status"], (A.shape, scale)
        assert warm["pivots"][0] == first["pivots"][0]
        assert warm["pivots"][1] <= sum(scratch["pivots"]), (A.shape, scale)
        assert warm["phase"] == (2 if warm["status"] == oracle.FEASIBLE else 3)
        if scratch["status"] == oracle.FEASIBLE:
            # the from-scratch objective is phase 1's residue plus c x; the warm one starts from y b
            left = max(abs(warm["opt"] - scratch["opt"]) - _phase1_residue(A, b2, c), 0.0)
            worst = max(worst, left / abs(scratch["opt"]))
        most = max(most, warm["dual"])
    return worst, most


def test_warm_start_against_scratch():
    """prints the largest relative objective difference (DESIGN.md §10.4 quotes it).  The bound: both
    solves end at an eps-optimal vertex, the same one here, so beyond the from-scratch solve's phase-1
    residue (|d[0]| < eps after phase 1, kept by phase 2; up to 4.4e-11 at (4, 513), where the
    right-hand sides sum to 2.6e4) only rounding is left"""
    worst = 0.0
    for n, m in WARM_SHAPES:
        for scale in HOST_SCALES:
            worst = max(worst, _against_scratch(warm_instances(n, m), scale)[0])
    for n, m in RHS_SHAPES:
        for scale in HOST_SCALES:
            w, most = _against_scratch(rhs_instances(n, m), scale)
            worst = max(worst, w)
            if scale == 1.0 and (n, m) != (1, 1):
                assert most >= 1, (n, m)  # the GPU file's warm batches pivot in the dual loop
    print(f"warm re-rhs: largest relative objective difference beyond the phase-1 residue {worst:.3e}")
    assert worst <= ROUNDING


def test_negated_row_is_infeasible_both_ways():
    pivots = []
    for n, m in RHS_SHAPES:
        for k, (A, b, c) in enumerate(rhs_instances(n, m)):
            b2 = negated_rhs(b, k + 1)
            warm = ref_rhs(ref_state(A, b, c), A, b2, c)
            assert warm["status"] == oracle.INFEASIBLE and warm["phase"] == 3
            assert ref_state(A, b2, c)["status"] == oracle.INFEASIBLE
            assert np.isnan(warm["opt"]) and not bits(warm["x"]).any()
            pivots.append(warm["pivots"][1])
    assert max(pivots) >= 1


@pytest.mark.parametrize("n,m", [(20, 10), (33, 31), (600, 4)])
def test_cap_then_resume_is_the_whole_solve(n, m):
    insts = rhs_instances(n, m)
    for (A, b, c), b2 in zip(insts, scaled_batch(insts, 1.0)):
        first = ref_state(A, b, c)
        whole = ref_rhs(first, A, b2, c)
        for cap in [0] + RHS_CAPS:
            capped = ref_rhs(first, A, b2, c, cap)
            if whole["pivots"][1] > cap:
                assert (capped["status"], capped["phase"], capped["pivots"][1]) == (oracle.PIVOT_CAP, 3, cap)
            same_fields(ref_rhs_resume(capped, c), whole)
            same_fields(ref_rhs_resume(capped, c, cap), capped)
        same_fields(ref_rhs_resume(whole, c), whole)
        # a second re-rhs on the result, back to the first right-hand side
        again = ref_rhs(whole, A, b, c)
        assert again["status"] == oracle.FEASIBLE and again["pivots"][0] == first["pivots"][0]
        # INFEASIBLE inside the dual loop ends again without a pivot
        bad = ref_rhs(first, A, negated_rhs(b, 1), c)
        assert bad["phase"] == 3
        same_fields(ref_rhs_resume(bad, c), bad)


def test_ladder_depends_on_the_combine_order():
    """the eps-argmin tree's leaving row is not the first exact minimum's on the ladder cases: the
    pivot path, and with it a compared field, differs.  (The entering ratio has no such case here:
    its candidates d[j] / -T[r][j] cannot be set through b'.)"""
    statuses = set()
    for (A, b, c), b2 in ladder_cases():
        first = ref_state(A, b, c)
        tree = ref_rhs(first, A, b2, c)
        plain = ref_rhs(first, A, b2, c, argmin=first_min)
        assert tree["dual"] >= 1
        assert tree["pivots"] != plain["pivots"] or not np.array_equal(tree["base"], plain["base"])
        statuses.add(tree["status"])
    assert statuses == {oracle.FEASIBLE, oracle.INFEASIBLE}
