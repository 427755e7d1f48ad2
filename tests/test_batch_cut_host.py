"""Gomory mixed-integer cuts from a kept batch state (simplex_solve_batch_device_cut), host side only (no
GPU): the entry's return codes, which are decided before any device is touched, the Python wrapper's
validation, and the specification itself checked on the oracle alone -- batch_cut_refs.py restates the
entry from batch_rows_refs.ref_rows, the oracle's eps-argmin tree and the oracle's fma, and the GPU file
compares the kernel with that restatement bit for bit, so what the restatement claims is shown here:

  a cut excludes the kept optimum by the fractional part f0 of its source row
  no integer feasible point of a small integer program violates a cut of up to eight successive rounds,
  and the LP bound neither rises nor falls below the enumerated integer optimum
  the same for a mixed mask on sampled points whose masked coordinates are integral
  every shape of the GPU file has an instance with a real cut and a case with a null row
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_cut_refs import (AWAY, SCALES, frac, grown_arrays, masks, mixed_cut_instances, ref_cut, usable, want_cut)
from batch_rows_refs import rows_shapes
from batch_state_refs import ref_state
from device_entries import cut_struct
from simplexoncuda_amd import _lib

# Measured by the tests below (they print the figures); each bound leaves a margin of 100 over its figure.
CUT_OFF_MEASURED = 7.7e-14     # |cut_A x* - cut_b - f0|, absolute (7.638e-14)
VIOLATION_MEASURED = 1.5e-14   # cut_A p - cut_b over the integer (or mask-integral) feasible points p, absolute (1.421e-14)
BOUND_MEASURED = 4.5e-16       # the LP bound below the integer optimum, relative to the bound (4.438e-16); no bound
#                                ever rose (the smallest fall of a round is 4.0e-5 of the bound), so a rise gets the same


# ------------------------------------------------------------------ return codes
def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host): three
    problems of the grown shape (20, 11), the source holding 10 rows"""
    base = dict(n=20, m=11, count=3, A=8, A_sb=220, A_sr=20, A_sc=1, b=8, b_sb=11, b_si=1, c=8, c_sb=20, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _cut(**kw):
    base = dict(cuts=1, away=0.05, integer=8, integer_sb=0, integer_sj=1, row=None, cut_A=8, cut_A_sb=220, cut_A_sr=20,
                cut_A_sc=1, cut_b=8, cut_b_sb=11, cut_b_si=1, cut_row=8)
    base.update(kw)
    return cut_struct(**base)


def _call(args, sin=None, sout=None, cut=None):
    lib = _lib.load()
    ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
    return lib.simplex_solve_batch_device_cut(ref(args), ref(sin), ref(sout), ref(cut))


def test_cut_entry_argument_checks():
    """the rows entry's codes in its order, with the entry's own: -3 for cuts and away, -2 for the struct
    and its four required arrays, -4 for the written strides and the mask's; none needs a device"""
    assert _call(None) == -1
    assert _call(None, _state(), _state(2), _cut()) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=-1), _state(), None, _cut()) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=-1), _state(), None, _cut(cuts=0)) == -1
    assert _call(_lib.BatchDeviceT(n=1, m=721, count=4), _state(), _state(2), _cut()) == -3  # a bad shape
    assert _call(_lib.BatchDeviceT(n=0, m=3, count=4), _state(), None, _cut()) == -3
    # cuts out of range (no cut, or no row left for the in-state), away outside (0, 0.5]
    empty = _lib.BatchDeviceT(n=20, m=11, count=0)
    for bad in (dict(cuts=0), dict(cuts=-1), dict(cuts=11), dict(cuts=12), dict(away=0.0), dict(away=-0.05),
                dict(away=0.5000001), dict(away=1.0), dict(away=float("nan")), dict(away=float("inf"))):
        assert _call(_args(), _state(), _state(2), _cut(**bad)) == -3, bad
        assert _call(empty, _state(), _state(2), _cut(**bad)) == -3, bad
    assert _call(_args(), _state(), _state(2), _cut(cuts=10, away=0.5)) == -5
    # an empty call
    assert _call(empty, _state(), _state(2), _cut()) == 0
    assert _call(empty, None, None, None) == 0
    # the struct and its four required arrays; row is optional
    assert _call(_args(), _state(), _state(2), None) == -2
    for f in ("integer", "cut_A", "cut_b", "cut_row"):
        assert _call(_args(), _state(), _state(2), _cut(**{f: None})) == -2, f
    assert _call(_args(), _state(), _state(2), _cut(row=8)) == -5
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=3), _state(), None, _cut()) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), _state(), _state(2), _cut()) == -2, f
    # `in` is required
    assert _call(_args(), None, _state(2), _cut()) == -2
    assert _call(_args(), None, None, _cut()) == -2
    # a NULL member of a state struct that is passed
    for f in ("T", "d", "base", "phase", "pivots"):
        bad = _state()
        setattr(bad, f, None)
        assert _call(_args(), bad, _state(2), _cut()) == -2, f
        assert _call(_args(), bad, None, _cut()) == -2, f
        bad = _state(2)
        setattr(bad, f, None)
        assert _call(_args(), _state(), bad, _cut()) == -2, f
    # `out` shares a member with `in`: the shapes differ, so in place is impossible
    assert _call(_args(), _state(), _state(), _cut()) == -2
    for f in ("T", "d", "base", "phase", "pivots"):
        shared = _state(2)
        setattr(shared, f, 1)
        assert _call(_args(), _state(), shared, _cut()) == -2, f
    # A, b and c are required and every stride is checked
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), _state(), _state(2), _cut()) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), _state(), _state(2), _cut()) == -4, f
    # the outputs' strides along a dimension longer than 1, and the mask's over the variables
    for f in ("cut_A_sb", "cut_A_sc", "cut_b_sb", "integer_sj"):
        assert _call(_args(), _state(), _state(2), _cut(**{f: 0})) == -4, f
    for f in ("cut_A_sr", "cut_b_si"):
        assert _call(_args(), _state(), _state(2), _cut(**{f: 0})) == -5, f         # one cut: a row stride of 0
        assert _call(_args(), _state(), _state(2), _cut(cuts=2, **{f: 0})) == -4, f
    assert _call(_args(), _state(), None, _cut(integer_sb=0)) == -5  # one mask for every problem
    # a missing required pointer comes before the strides, the source's before the entry's own, all before -5
    assert _call(_args(status=None, A_sr=0), _state(), None, _cut(cut_A_sc=0)) == -2
    assert _call(_args(), _state(), None, _cut(cut_A=None, cut_A_sc=0)) == -2
    assert _call(_args(A=None), _state(), None, _cut(cut_A_sc=0)) == -2
    # ... and then every check up to the workspace's is passed
    assert _call(_args(), _state(), _state(2), _cut()) == -5
    assert _call(_args(), _state(), None, _cut()) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20), _state(), None, _cut()) == -5   # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255), _state(), None, _cut()) == -5    # no header


def test_source_is_checked_against_the_in_states_rows():
    """the row dimension of A and b has the in-state's length m - cuts: a source of one row may have row
    strides of 0 where the rows entry's check, made with m, says otherwise; a stride of 0 along a dimension
    of length 1 is accepted everywhere, as in the device entry"""
    one_row = dict(A_sr=0, b_si=0)
    assert _call(_args(**one_row), _state(), None, _cut(cuts=10)) == -5  # m0 = 1
    assert _call(_args(**one_row), _state(), None, _cut(cuts=9)) == -4   # m0 = 2
    one = dict(n=1, m=2, count=1, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0, c_sb=0, c_sj=0)
    zero = dict(cut_A_sb=0, cut_A_sr=0, cut_A_sc=0, cut_b_sb=0, cut_b_si=0, integer_sj=0)
    assert _call(_args(**one), _state(), None, _cut(**zero)) == -5


def test_wrapper_validates_before_any_device_use():
    cpu = torch.device("cpu")
    s = sx.BatchState.empty(3, 5, 4, cpu)
    f64 = dict(dtype=torch.float64)
    A, b, c = torch.ones((3, 6, 5), **f64), torch.ones((3, 6), **f64), torch.ones((3, 5), **f64)
    mask = torch.ones(5, dtype=torch.bool)
    call = sx.cut_batch_tensors
    with pytest.raises(TypeError, match="must be a BatchState"):
        call(None, A, b, c, mask, cuts=2)
    with pytest.raises(TypeError, match="c must be a torch.Tensor"):
        call(s, A, b, None, mask, cuts=2)
    with pytest.raises(TypeError, match="float64"):
        call(s, A, b.to(torch.float32), c, mask, cuts=2)
    with pytest.raises(ValueError, match="c must be"):
        call(s, A, b, c[:, :4], mask, cuts=2)
    with pytest.raises(ValueError, match="state.T must be a contiguous"):
        call(sx.BatchState(s.T[:, :3], s.d, s.base, s.phase, s.pivots, 5, 4), A, b, c, mask, cuts=2)
    for cuts in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="cuts must be an int >= 1"):
            call(s, A, b, c, mask, cuts=cuts)
    for away in (0.0, 0.6, float("nan"), 1):
        with pytest.raises(ValueError, match="away must be a float in"):
            call(s, A, b, c, mask, cuts=2, away=away)
    # A and b hold the state's rows and one more per cut, no other number
    for cuts in (1, 3):
        with pytest.raises(ValueError, match="the state's 4 rows and"):
            call(s, A, b, c, mask, cuts=cuts)
    with pytest.raises(ValueError, match="so b must be"):
        call(s, A, b[:, :5], c, mask, cuts=2)
    with pytest.raises(TypeError, match="integer must be a torch.Tensor"):
        call(s, A, b, c, [1] * 5, cuts=2)
    with pytest.raises(TypeError, match="integer must be bool or uint8"):
        call(s, A, b, c, mask.to(torch.int32), cuts=2)
    for bad in (torch.ones(4, dtype=torch.bool), torch.ones((2, 5), dtype=torch.bool), torch.ones((3, 5, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"integer must be \[5\] or \[3, 5\]"):
            call(s, A, b, c, bad, cuts=2)
    with pytest.raises(TypeError, match="rows must be a torch.Tensor"):
        call(s, A, b, c, mask, cuts=2, rows=[[0, 1]] * 3)
    with pytest.raises(TypeError, match="rows must be int32"):
        call(s, A, b, c, mask, cuts=2, rows=torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"rows must be \[3, 2\]"):
        call(s, A, b, c, mask, cuts=2, rows=torch.zeros((3, 1), dtype=torch.int32))
    # A and b are written: no zero stride along a dimension longer than 1
    with pytest.raises(ValueError, match="A is written"):
        call(s, A[:1].expand(3, 6, 5), b, c, mask, cuts=2)
    with pytest.raises(ValueError, match="b is written"):
        call(s, A, b[:, :1].expand(3, 6), c, mask, cuts=2)
    with pytest.raises(ValueError, match="must be on a GPU"):
        call(s, A, b, c, mask, cuts=2)
    # the other paths leave the new attribute None, and the constructors' positional use still works
    assert sx.BatchTensors(1, 2, 3, 4, 5, 6, 7, 8).cut_rows is None
    assert sx.BatchTensors(1, 2, 3, 4, 5, 6, 7, 8, None, None, s).state is s


# ------------------------------------------------------------------ the restatement on the oracle
def _family():
    """((n, m0, q), scale, inst, kept state, ref_cut) over every shape of the GPU file and both scales of b,
    all-integer mask"""
    for n, m0, q in rows_shapes():
        for scale in SCALES:
            for inst, ref, want in zip(*want_cut(n, m0, q, scale)):
                yield (n, m0, q), scale, inst, ref, want


def test_coverage_of_the_family():
    """a condition on the instances, not a measurement: at every shape at least one instance yields a real
    cut and at least one case a null row (the none mask always does; so does q = 3 where fewer than three
    rows qualify), and over the whole family at most 20 % of the instances yield null rows only"""
    real, null = {}, {}
    total = null_only = 0
    for shape, scale, inst, ref, (cut_A, cut_b, cut_row, grown) in _family():
        assert ref["status"] == oracle.FEASIBLE and usable(ref, shape[2])
        total += 1
        null_only += not (cut_row >= 0).any()
        real[shape] = real.get(shape, 0) + int((cut_row >= 0).any())
        null[shape] = null.get(shape, 0) + int((cut_row < 0).any())
        for t in np.flatnonzero(cut_row < 0):
            assert not cut_A[t].view(np.uint64).any() and not cut_b[t:t + 1].view(np.uint64).any()
    for n, m0, q in rows_shapes():
        assert real[(n, m0, q)] >= 1, (n, m0, q)
        none = ref_cut(ref_state(*want_cut(n, m0, q, 37)[0][0]), *want_cut(n, m0, q, 37)[0][0], masks(n)["none"], q)
        assert (none[2] == -1).all() and not none[0].view(np.uint64).any() and none[3]["dual"] == 0
        null[(n, m0, q)] += 1
        assert null[(n, m0, q)] >= 1
    assert null[(5, 4, 3)] >= 2  # a null row behind real ones
    print(f"null-only instances: {null_only} of {total}")
    assert total == 60 and null_only <= 0.2 * total


def test_cut_excludes_the_kept_optimum_by_f0():
    """cut_A x* - cut_b = f0 of the source row, which lies in [away, 1 - away]; the grown LP stays FEASIBLE
    and the dual loop pivots.  Prints the largest deviation"""
    worst = 0.0
    cuts = 0
    for (n, m0, q), scale, inst, ref, (cut_A, cut_b, cut_row, grown) in _family():
        assert grown["status"] == oracle.FEASIBLE and grown["phase"] == 2
        assert (grown["dual"] >= 1) == bool((cut_row >= 0).any())
        assert len(set(cut_row[cut_row >= 0])) == (cut_row >= 0).sum()  # different source rows
        for t in np.flatnonzero(cut_row >= 0):
            f0 = frac(ref["T"][cut_row[t], 0])
            assert AWAY <= f0 <= 1.0 - AWAY and ref["base"][cut_row[t]] < n
            worst = max(worst, abs(float(cut_A[t] @ ref["x"]) - cut_b[t] - f0))
            cuts += 1
    print(f"cut-off: {cuts} cuts, largest |cut_A x* - cut_b - f0| {worst:.3e}")
    assert cuts >= 50
    assert worst <= 100 * CUT_OFF_MEASURED


# ---- validity on small integer programs, by enumeration
def _small_programs():
    """generated instances in [1, 100] with n <= 5 whose b is scaled by 5 .. 10, so that the box holds more
    than the origin: those with 3 to 500 integer feasible points, and those points"""
    progs = []
    for n, m, seed in itertools.product((2, 3, 4, 5), (2, 3, 4), (11, 12, 13)):
        A, b, c = oracle.generate(n, m, 1000 * seed + 100 * n + m, 1, 100)
        b = b * float(5 + (seed + n + m) % 6)
        ub = [int(np.floor((b / A[:, j]).min())) for j in range(n)]
        pts = np.array([p for p in itertools.product(*(range(u + 1) for u in ub)) if (A @ np.array(p, dtype=float) <= b).all()],
                       dtype=np.float64)
        if 3 <= len(pts) <= 500:
            progs.append((A, b, c, pts))
    return progs


def _rounds(A, b, c, mask, pts, rounds=8):
    """up to `rounds` successive single cuts of one program: (cuts made, the largest violation of a cut by
    one of pts, the largest rise of the bound, the largest fall of the bound below the best of pts), the last
    two relative to the bound"""
    best = float((pts @ c).max())
    state = ref_state(A, b, c)
    assert state["status"] == oracle.FEASIBLE
    made, viol, rise, fall = 0, -np.inf, -np.inf, -np.inf
    for _ in range(rounds):
        bound = state["opt"]
        fall = max(fall, (best - bound) / abs(bound))
        cut_A, cut_b, cut_row, grown = ref_cut(state, A, b, c, mask, 1)
        if cut_row[0] < 0:
            break
        made += 1
        viol = max(viol, float((pts @ cut_A[0] - cut_b[0]).max()))
        assert grown["status"] == oracle.FEASIBLE and grown["phase"] == 2 and grown["dual"] >= 1
        rise = max(rise, (grown["opt"] - bound) / abs(bound))
        A, b, _ = grown_arrays((A, b, c), (cut_A, cut_b))
        state = grown
    return made, viol, rise, fall


def test_no_integer_point_violates_a_cut():
    """every integer feasible point of at least 15 small integer programs is enumerated; no cut of up to 8
    successive rounds -- from the second on the source rows carry earlier cuts' slacks -- is violated by one,
    and the LP bound never rises and never falls below the enumerated integer optimum.  Prints the largest
    violation, rise and fall"""
    progs = _small_programs()
    assert len(progs) >= 15 and all(A.shape[1] <= 5 for A, _, _, _ in progs)
    cuts, viol, rise, fall = 0, -np.inf, -np.inf, -np.inf
    later = 0
    for A, b, c, pts in progs:
        made, v, r, f = _rounds(A, b, c, masks(A.shape[1])["all"], pts)
        cuts += made
        later += made >= 2
        viol, rise, fall = max(viol, v), max(rise, r), max(fall, f)
    print(f"validity: {len(progs)} programs, {cuts} cuts, largest violation {viol:.3e}, rise {rise:.3e}, fall {fall:.3e}")
    assert cuts >= 2 * len(progs) and later >= 10  # chained rounds are the rule, not the exception
    assert viol <= 100 * VIOLATION_MEASURED
    assert rise <= 100 * BOUND_MEASURED and fall <= 100 * BOUND_MEASURED


def test_mixed_mask_on_sampled_points():
    """every second variable integer: the cuts hold at sampled feasible points whose masked coordinates are
    integral (the others are not), over the same programs and rounds, and the bound never rises and never
    falls below the best sampled point"""
    progs = _small_programs()
    rng = np.random.default_rng(20240)
    cuts, viol, rise, fall, sampled = 0, -np.inf, -np.inf, -np.inf, 0
    for A, b, c, _ in progs:
        n = A.shape[1]
        mask = masks(n)["second"]
        ub = np.array([(b / A[:, j]).min() for j in range(n)])
        pts = rng.uniform(0.0, 1.0, size=(4000, n)) * ub
        pts[:, mask] = np.floor(pts[:, mask])
        pts = pts[(pts @ A.T <= b).all(axis=1)]
        assert len(pts) >= 20
        sampled += len(pts)
        made, v, r, f = _rounds(A, b, c, mask, pts)
        cuts += made
        viol, rise, fall = max(viol, v), max(rise, r), max(fall, f)
    print(f"mixed mask: {sampled} points, {cuts} cuts, largest violation {viol:.3e}, rise {rise:.3e}, fall {fall:.3e}")
    assert cuts >= 15  # (fewer rows qualify than with every variable integer)
    assert viol <= 100 * VIOLATION_MEASURED
    assert rise <= 100 * BOUND_MEASURED and fall <= 100 * BOUND_MEASURED


def test_states_that_are_not_kept_optima_get_null_rows():
    """phase-1 states and UNBOUNDED phase-2 states of the mixed batch are not usable: null rows, and the rows
    entry's cold start on the problem with them"""
    cold = warm = 0
    for A0, b0, c in mixed_cut_instances():
        st = ref_state(A0, b0, c)
        cut_A, cut_b, cut_row, grown = ref_cut(st, A0, b0, c, masks(12)["all"], 2)
        if usable(st, 2):
            warm += 1
            assert st["status"] == oracle.FEASIBLE and "dual" in grown
            continue
        cold += 1
        assert (st["phase"], st["status"]) in ((1, oracle.INFEASIBLE), (2, oracle.UNBOUNDED))
        assert (cut_row == -1).all() and not cut_A.view(np.uint64).any() and not cut_b.view(np.uint64).any()
        assert "dual" not in grown
    assert cold >= 2 and warm >= 2
