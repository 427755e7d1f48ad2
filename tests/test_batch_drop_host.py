"""Rows or columns taken out of a kept batch state (simplex_solve_batch_device_drop), host side only (no
GPU): the entry's return codes, which are decided before any device is touched, the Python wrappers'
validation, and the specification itself checked on the oracle alone -- batch_drop_refs.py restates the
entry from the oracle's argmin, ratio and pivot and batch_rhs_refs' loops, and the GPU file compares the
kernel with that restatement bit for bit, so what the restatement claims is shown here:

  a drop reaches the from-scratch solve's status on the reduced problem and its optimum
  the right-hand-side entry's identities T[:, 0] = S b and d[0] = y b hold on the reduced state
  every path is taken: none, forced+, forced-, forced-dual, and cold by a selection without a candidate
  a loose cut or a column that does not price in, added and dropped again, gives the kept state back
  a capped run behind the forced pivots resumed is the uncapped one; a chain of entries follows
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_cols_refs import ref_cols
from batch_drop_refs import (CAP_COLS, CAP_ROWS, COLS, DROP_CAPS, ROUND_TRIP_SHAPES, ROWS, added_col, added_row,
                             candidates, column_0_batch, forced_minus_instance, handmade, in_class, many_drops,
                             mixed_batch, reduced, ref_drop, shapes, want_batch)
from batch_rhs_refs import new_rhs, ref_rhs, ref_rhs_resume
from batch_rows_refs import make_row, ref_rows
from batch_state_refs import ref_state, same_fields, warm_instances
from simplexoncuda_amd import _lib

# Rounding alone, relative to the optimum: the project's bound for a warm start that reaches the same
# vertex by another pivot path (test_batch_state_host.py and the files of the later state entries).
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


def _call(args, sin=None, sout=None, kind=0, dropped=1, idx=8):
    lib = _lib.load()
    return lib.simplex_solve_batch_device_drop(None if args is None else ctypes.byref(args),
                                               None if sin is None else ctypes.byref(sin),
                                               None if sout is None else ctypes.byref(sout), kind, dropped, idx)


def test_drop_entry_argument_checks():
    """the rows entry's codes in its order, with A, b, c and idx always required, `out` never `in`, kind in
    {0, 1}, dropped >= 1, and the class taken from the in-state's shape; none needs a device"""
    assert _call(None) == -1
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=-1), _state()) == -1
    for kind in (0, 1):
        assert _call(_lib.BatchDeviceT(n=3, m=0, count=4), _state(), None, kind) == -3  # a reduced dimension below 1
        assert _call(_lib.BatchDeviceT(n=0, m=3, count=4), _state(), None, kind) == -3
    # the in-state's shape decides the class: (2, 720) is resident, (2, 721) is not
    assert sx.batch_class(2, 720) == 1 and sx.batch_class(2, 721) == 0
    assert _call(_lib.BatchDeviceT(n=2, m=720, count=4), _state(), _state(2), 0, 1) == -3
    assert _call(_lib.BatchDeviceT(n=2, m=700, count=4), _state(), _state(2), 0, 21) == -3
    assert _call(_lib.BatchDeviceT(n=2, m=719, count=0), _state(), _state(2), 0, 1) == 0
    assert _call(_lib.BatchDeviceT(n=2, m=720, count=0), _state(), _state(2), 0, 1) == -3
    assert _call(_lib.BatchDeviceT(n=2, m=720, count=4), _state(), _state(2), 1, 2 ** 31 - 2) == -3
    for kind in (-1, 2, 3):
        assert _call(_args(), _state(), _state(2), kind) == -3, kind
        assert _call(_lib.BatchDeviceT(n=21, m=10, count=0), _state(), _state(2), kind) == -3, kind
    for dropped in (0, -1):
        for kind in (0, 1):
            assert _call(_args(), _state(), _state(2), kind, dropped) == -3, dropped
            assert _call(_lib.BatchDeviceT(n=21, m=10, count=0), _state(), _state(2), kind, dropped) == -3, dropped
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=0), _state(), _state(2)) == 0
    assert _call(_lib.BatchDeviceT(n=21, m=10, count=3), _state()) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), _state(), _state(2)) == -2, f
    # `in` and idx are required
    assert _call(_args(), None, _state(2)) == -2
    assert _call(_args(), None, None) == -2
    for kind in (0, 1):
        assert _call(_args(), _state(), _state(2), kind, 1, None) == -2
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
    # A, b and c are required and every stride is checked, against the reduced shape
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), _state(), _state(2)) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), _state(), _state(2)) == -4, f
    # ... and then every check up to the workspace's is passed
    for kind in (0, 1):
        for dropped in (1, 3):
            assert _call(_args(), _state(), _state(2), kind, dropped) == -5
            assert _call(_args(), _state(), None, kind, dropped) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20), _state(), None) == -5   # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255), _state(), None) == -5    # no header
    # a stride of 0 along a dimension of length 1 of the reduced shape is accepted, whatever the in-state's
    one = dict(n=1, m=1, count=1, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0, c_sb=0, c_sj=0)
    assert _call(_args(**one), _state(), None, 0) == -5
    assert _call(_args(**one), _state(), None, 1) == -5


def test_wrappers_validate_before_any_device_use():
    f64 = dict(dtype=torch.float64)
    s = sx.BatchState.empty(3, 5, 4, torch.device("cpu"))
    one = torch.zeros((3, 1), dtype=torch.int32)
    for fn, A, b, c in ((sx.drop_rows_batch_tensors, torch.ones((3, 3, 5), **f64), torch.ones((3, 3), **f64),
                         torch.ones((3, 5), **f64)),
                        (sx.drop_cols_batch_tensors, torch.ones((3, 4, 4), **f64), torch.ones((3, 4), **f64),
                         torch.ones((3, 4), **f64))):
        with pytest.raises(TypeError, match="must be a BatchState"):
            fn(None, one, A, b, c)
        with pytest.raises(TypeError, match="c must be a torch.Tensor"):
            fn(s, one, A, b, None)
        with pytest.raises(TypeError, match="must be a torch.Tensor"):
            fn(s, [[0]] * 3, A, b, c)
        with pytest.raises(TypeError, match="must be int32"):
            fn(s, one.to(torch.int64), A, b, c)
        with pytest.raises(ValueError, match=r"must be \[3, q\]"):
            fn(s, one[0], A, b, c)
        with pytest.raises(ValueError, match=r"must be \[3, q\]"):
            fn(s, one[:2], A, b, c)
        with pytest.raises(ValueError, match=r"must be \[3, q\]"):
            fn(s, one[:, :0], A, b, c)
        with pytest.raises(TypeError, match="float64"):
            fn(s, one, A, b.to(torch.float32), c)
        with pytest.raises(ValueError, match="c must be"):
            fn(s, one, A, b, c[:2])
        with pytest.raises(ValueError, match="state.T must be a contiguous"):
            fn(sx.BatchState(s.T[:, :3], s.d, s.base, s.phase, s.pivots, 5, 4), one, A, b, c)
        with pytest.raises(ValueError, match="leaves none"):
            fn(s, torch.zeros((3, 5), dtype=torch.int32), A, b, c)
        # A, b and c are the reduced problem's
        with pytest.raises(ValueError, match="the reduced problem"):
            fn(s, one, torch.ones((3, 4, 5), **f64), torch.ones((3, 4), **f64), torch.ones((3, 5), **f64))
        with pytest.raises(ValueError, match="the reduced problem"):
            fn(s, torch.zeros((3, 2), dtype=torch.int32), A, b, c)
        with pytest.raises(ValueError, match="must be on a GPU"):
            fn(s, one, A, b, c)


def test_shapes_the_gpu_file_relies_on():
    """the class of a launch is the in-state's shape's: (241, 64 -> 63) and (241 -> 240, 64) work in a
    workspace slice and leave an LDS-class state, (241, 65 -> 64) and (242 -> 241, 64) stay in the workspace
    class; (4, 513 -> 512) selects its forced row over two tiles and everything behind over one; the forced
    dual selection of (513 -> 512, 4) has 517 candidates and that of (512 -> 511, 4) 516, those behind them
    516 and 515; the in-state's dense stride comes in both parities"""
    assert in_class(ROWS, 64, 64, 1) == (2, 2) and in_class(COLS, 64, 64, 1) == (2, 2)
    assert in_class(ROWS, 241, 64, 1) == (1, 2) and in_class(ROWS, 241, 65, 1) == (1, 1)
    assert in_class(COLS, 241, 64, 1) == (1, 2) and in_class(COLS, 242, 64, 1) == (1, 1)
    assert in_class(ROWS, 4, 513, 1) == (1, 1) and in_class(COLS, 5, 513, 1) == (1, 1)
    assert in_class(ROWS, 600, 5, 1) == (2, 2) and in_class(COLS, 600, 4, 1) == (2, 2)
    for kind in (ROWS, COLS):
        assert len(set(shapes(kind))) == len(shapes(kind))
        assert {(1 + n + m) % 2 for n, m, _ in shapes(kind)} == {0, 1}
        assert any(q == 3 for _, _, q in shapes(kind))
    assert len(shapes(ROWS)) == 10 and len(shapes(COLS)) == 12


# ------------------------------------------------------------------ the restatement on the oracle
def _cases():
    """(kind, shape, insts, refs, lists, reduced instances, want) over both kinds and every shape"""
    for kind in (ROWS, COLS):
        for shape in shapes(kind):
            yield (kind, shape) + want_batch(kind, *shape)


def test_paths_are_covered():
    """every shape's batch holds a drop without arithmetic and a forced one, in one list where q = 3; the
    in-states are FEASIBLE phase-2 states and none of these cases is cold.  forced- and the selections
    without a candidate are not reached by generated instances: test_forced_minus, test_no_candidate"""
    count = {}
    for kind, shape, _, refs, lists, _, want in _cases():
        assert all(r["status"] == oracle.FEASIBLE and r["phase"] == 2 for r in refs), shape
        assert all(w["why"] is None and len(w["paths"]) == shape[2] for w in want), shape
        taken = {p for w in want for p in w["paths"]}
        assert "none" in taken and taken & {"forced+", "forced-", "forced-dual"}, (kind, shape, taken)
        if shape[2] == 3:
            assert any(len(set(w["paths"])) > 1 for w in want), shape
        for w in want:
            assert w["pivots"][1] >= w["forced"] == sum(p != "none" for p in w["paths"])
            for p in w["paths"]:
                count[(kind, p)] = count.get((kind, p), 0) + 1
    print(f"paths over the generated set: {count}")
    assert set(count) == {(ROWS, "none"), (ROWS, "forced+"), (COLS, "none"), (COLS, "forced-dual")}


def test_drop_against_scratch():
    """the same status as oracle.two_phase on the reduced problem in every case, and the same optimum to
    the project's bound for two pivot paths to one vertex.  A from-scratch solve keeps its phase-1 residue
    in d[0]; the drop keeps the kept state's.  Measured (printed): 8.8e-12 relative as it stands, at
    (5 -> 4, 513), and 7.6e-16 with the two residues set aside"""
    worst = worst_left = 0.0
    cases = 0
    for kind, shape, insts, refs, lists, small, want in _cases():
        for inst, g, w in zip(insts, small, want):
            cases += 1
            scratch = oracle.two_phase(*g)
            assert w["status"] == scratch["status"] == oracle.FEASIBLE, (kind, shape)
            diff = abs(w["opt"] - scratch["opt"])
            residue = abs(scratch["phase1_value"]) + abs(oracle.two_phase(*inst)["phase1_value"])
            worst = max(worst, diff / abs(scratch["opt"]))
            worst_left = max(worst_left, max(diff - residue, 0.0) / abs(scratch["opt"]))
    print(f"drops, {cases} cases: largest relative objective difference {worst:.3e}, {worst_left:.3e} beyond the "
          "phase-1 residues")
    assert cases == 66
    assert worst <= ROUNDING


def test_identities():
    """T[:, 0] = S b and d[0] = y b on every reduced phase-2 state, S its slack block, y the slack entries
    of d and b the reduced right-hand side (batch_rhs_refs.new_rhs): the column relative to its largest
    entry, the objective relative to itself with the kept state's phase-1 residue set aside.  Measured
    (printed): 5.7e-15 for the column and 1.8e-15 for the objective; asserted at 100 times that"""
    worst_col = worst_obj = 0.0
    states = 0
    for kind, shape, insts, refs, lists, small, want in _cases():
        for inst, (A, b, c), st in zip(insts, small, want):
            assert st["phase"] == 2
            states += 1
            col, obj = new_rhs(st, b)
            worst_col = max(worst_col, np.abs(col - st["T"][:, 0]).max() / max(np.abs(st["T"][:, 0]).max(), 1.0))
            residue = abs(oracle.two_phase(*inst)["phase1_value"])
            worst_obj = max(worst_obj, max(abs(obj - st["d"][0]) - residue, 0.0) / max(abs(st["d"][0]), 1.0))
    print(f"identities on the reduced state, {states} states: column {worst_col:.3e}, objective {worst_obj:.3e}")
    assert states == 66
    assert worst_col <= 5.7e-13 and worst_obj <= 1.8e-13


def test_forced_minus():
    """the issue's instance: the optimum (4, 5) has row 0 tight, slack 0's column is (-1, 0), so the slack
    moves down; the reduced optimum is 5 at (0, 5), as from scratch"""
    inst = forced_minus_instance()
    st = ref_state(*inst)
    assert st["status"] == oracle.FEASIBLE and np.array_equal(st["x"], [4.0, 5.0])
    assert np.array_equal(st["T"][:, 3], [0.0, -1.0]) or np.array_equal(st["T"][:, 3], [-1.0, 0.0])
    g = reduced(inst, ROWS, [0])
    w = ref_drop(st, ROWS, [0], *g)
    scratch = oracle.two_phase(*g)
    assert w["paths"] == ["forced-"] and w["status"] == scratch["status"] == oracle.FEASIBLE
    assert w["opt"] == scratch["opt"] == 5.0 and np.array_equal(w["x"], [0.0, 5.0])
    assert (w["T"][:, 0] >= 0).all()


@pytest.mark.parametrize("kind", [ROWS, COLS])
def test_no_candidate(kind):
    """hand-made states (batch_drop_refs.handmade): the forced selection finds no candidate, the problem
    is cold and every field is the from-scratch solve's"""
    st, idx, g = handmade(kind)
    w = ref_drop(st, kind, idx, *g)
    assert w["why"] == "no-candidate" and w["path"] == "cold" and w["paths"] == []
    same_fields(w, ref_state(*g))
    want = oracle.two_phase(*g)
    want["row"] = oracle.last_objective_row().copy()
    same_fields(w, want, ("status", "pivots", "base", "row"))


def test_cold_and_warm_in_the_mixed_batch():
    """phase-1 in-states are cold: oracle.two_phase on the reduced problem in every field.  UNBOUNDED and
    FEASIBLE phase-2 in-states with a row dropped are warm and reach its status; with a basic column
    dropped the UNBOUNDED ones (not dual feasible) are cold"""
    seen = set()
    for kind in (ROWS, COLS):
        for k, inst in enumerate(mixed_batch()):
            st = ref_state(*inst)
            idx = [k % (10 if kind == ROWS else 12)]
            g = reduced(inst, kind, idx)
            w = ref_drop(st, kind, idx, *g)
            want = oracle.two_phase(*g)
            assert w["status"] == want["status"], (kind, k)
            seen.add((kind, st["phase"], st["status"], w["why"]))
            if w["why"]:
                want["row"] = oracle.last_objective_row().copy()
                same_fields(w, want, ("status", "pivots", "base", "row"))
            elif want["status"] == oracle.FEASIBLE:
                assert abs(w["opt"] - want["opt"]) <= ROUNDING * abs(want["opt"])
    print(sorted(seen, key=str))
    for kind in (ROWS, COLS):
        assert (kind, 1, oracle.INFEASIBLE, "phase-1") in seen
        assert (kind, 2, oracle.FEASIBLE, None) in seen and (kind, 2, oracle.UNBOUNDED, None) in seen
    assert (COLS, 2, oracle.UNBOUNDED, "dual-infeasible") in seen


def test_round_trips():
    """a loose cut (theta = 1.5) added and dropped again, and a column that does not price in (theta =
    0.01) added and dropped again, give the kept T, d and base back bit for bit without a pivot; a
    binding cut (theta = 0.5) added and dropped gives the status and the optimum to the bound"""
    for n, m in ROUND_TRIP_SHAPES:
        for inst in warm_instances(n, m)[:3]:
            st = ref_state(*inst)
            assert st["status"] == oracle.FEASIBLE
            loose = ref_rows(st, *added_row(inst, 1.5))
            back = ref_drop(loose, ROWS, [m], *inst)
            assert loose["pivots"][1] == 0 and back["paths"] == ["none"] and back["pivots"] == (st["pivots"][0], 0)
            same_fields(back, st, ("T", "d", "base", "phase", "status", "x", "opt", "row"))
            col = ref_cols(st, *added_col(inst, 0.01))
            back = ref_drop(col, COLS, [n], *inst)
            assert col["pivots"][1] == 0 and back["paths"] == ["none"]
            same_fields(back, st, ("T", "d", "base", "phase", "status", "x", "opt", "row"))
            tight = ref_rows(st, *added_row(inst, 0.5))
            back = ref_drop(tight, ROWS, [m], *inst)
            assert tight["pivots"][1] >= 1 and back["paths"] == ["forced+"] and back["status"] == oracle.FEASIBLE
            assert abs(back["opt"] - st["opt"]) <= ROUNDING * abs(st["opt"])


def test_phase_3_in_states():
    """in-states inside the dual loop.  The impossible row a x <= -1 of the rows entry, a generated
    positive a: its slack is the only negative right-hand side, so the dual loop's first pivot takes it out
    of the basis (in all 24 instances tried) and the state ends INFEASIBLE with that row tight.  So the warm
    drop of a basic slack is shown on the same row stopped by a cap of 0 (PIVOT_CAP inside the dual loop,
    the slack still basic) and on the row 0 x <= -1 (INFEASIBLE without a pivot): dropped again both are
    FEASIBLE with the kept T, d and base bit for bit.  The INFEASIBLE state's impossible row is the tight
    dropped row: cold.  A basic column with a positive value dropped from a phase-3 state (a binding cut
    stopped by a cap of 0) is warm and reaches the from-scratch optimum"""
    for inst in warm_instances(12, 10)[:3]:
        m, n = inst[0].shape
        st = ref_state(*inst)
        a, beta = make_row(inst, "never", 1.0)
        never = (np.vstack([inst[0], a]), np.append(inst[1], beta), inst[2])
        zero = (np.vstack([inst[0], np.zeros(n)]), np.append(inst[1], -1.0), inst[2])
        for stuck, status in ((ref_rows(st, *never, 0), oracle.PIVOT_CAP), (ref_rows(st, *zero), oracle.INFEASIBLE)):
            assert stuck["status"] == status and stuck["phase"] == 3 and stuck["pivots"][1] == 0
            assert (stuck["base"] == n + m).any()
            back = ref_drop(stuck, ROWS, [m], *inst)
            assert back["why"] is None and back["paths"] == ["none"] and back["pivots"] == (st["pivots"][0], 0)
            same_fields(back, st, ("T", "d", "base", "phase", "status", "x", "opt", "row"))
        stuck = ref_rows(st, *never)
        assert stuck["status"] == oracle.INFEASIBLE and stuck["phase"] == 3 and not (stuck["base"] == n + m).any()
        cold = ref_drop(stuck, ROWS, [m], *inst)
        assert cold["why"] == "phase-3"
        same_fields(cold, st)
        # its only basic structural variable stands in the infeasible row, which has no entry to pivot on
        (j,) = [int(v) for v in stuck["base"] if v < n]
        g = reduced(never, COLS, [j])
        w = ref_drop(stuck, COLS, [j], *g)
        assert w["why"] == "no-candidate" and w["status"] == oracle.two_phase(*g)["status"] == oracle.INFEASIBLE
        # a binding cut stopped by a cap of 0: a basic column with a positive value is forced out, the dual
        # loop goes on behind it
        cut = added_row(inst, 0.5)
        stuck = ref_rows(st, *cut, 0)
        assert stuck["status"] == oracle.PIVOT_CAP and stuck["phase"] == 3
        j = candidates(stuck, COLS)[1][0]
        g = reduced(cut, COLS, [j])
        w = ref_drop(stuck, COLS, [j], *g)
        want = oracle.two_phase(*g)
        assert w["why"] is None and w["paths"] == ["forced-dual"] and w["dual"] >= 1
        assert w["status"] == want["status"] == oracle.FEASIBLE and w["phase"] == 2
        assert abs(w["opt"] - want["opt"]) <= ROUNDING * abs(want["opt"])


def test_a_column_whose_removal_is_infeasible():
    """-x_0 <= -1 among the rows: without column 0 the row reads 0 <= -1.  Where x_0 > 1 stands in another
    row the forced dual pivot takes it out and the dual loop finds the row; where x_0 = 1 is basic in the
    new row itself that row offers no entering variable and the problem is cold.  From scratch agrees"""
    found = 0
    for big in column_0_batch():
        st = ref_state(*big)
        assert st["status"] == oracle.FEASIBLE and st["x"][0] >= 1.0 - 1e-9
        g = reduced(big, COLS, [0])
        w = ref_drop(st, COLS, [0], *g)
        assert w["status"] == oracle.two_phase(*g)["status"] == oracle.INFEASIBLE
        if st["x"][0] > 1.0 + 1e-6:
            found += 1
            assert w["paths"] == ["forced-dual"] and w["phase"] == 3 and w["dual"] == 0
        else:
            assert w["why"] == "no-candidate"
    assert found == 2


def test_cap_then_resume_and_a_chain():
    """behind the forced pivots a cap leaves PIVOT_CAP at max(cap, f) pivots and the resumed run is the
    uncapped one in every field; a row added, a column added, that row dropped, a new right-hand side and
    that column dropped each reach the from-scratch status"""
    for kind, shape in ((ROWS, CAP_ROWS), (COLS, CAP_COLS)):
        _, refs, lists, small, whole = want_batch(kind, *shape)
        assert max(w["pivots"][1] for w in whole) > 2
        for st, idx, g, w in zip(refs, lists, small, whole):
            for cap in [0] + DROP_CAPS:
                capped = ref_drop(st, kind, idx, *g, cap)
                assert capped["forced"] == w["forced"]
                if w["pivots"][1] > max(cap, w["forced"]):
                    assert capped["status"] == oracle.PIVOT_CAP and capped["pivots"][1] == max(cap, w["forced"])
                same_fields(ref_rhs_resume(capped, g[2]), w)
    for inst in warm_instances(32, 16)[:3]:
        n, m = 32, 16
        st = ref_state(*inst)
        g1 = added_row(inst, 0.5)
        s1 = ref_rows(st, *g1)
        g2 = added_col(g1, 100.0)
        s2 = ref_cols(s1, *g2)
        g3 = reduced(g2, ROWS, [m])
        s3 = ref_drop(s2, ROWS, [m], *g3)
        g4 = (g3[0], 1.05 * g3[1], g3[2])
        s4 = ref_rhs(s3, *g4)
        g5 = reduced(g4, COLS, [n])
        s5 = ref_drop(s4, COLS, [n], *g5)
        for s, g in ((s1, g1), (s2, g2), (s3, g3), (s4, g4), (s5, g5)):
            want = oracle.two_phase(*g)
            assert s["status"] == want["status"] == oracle.FEASIBLE
            assert abs(s["opt"] - want["opt"]) <= ROUNDING * abs(want["opt"])
        assert s5["T"].shape == (m, 1 + n + m)


def test_many_problems():
    """every twelfth of the 1,200 (5, 5 -> 4) problems, each dropping its own row: the from-scratch status,
    and both sorts of drop occur"""
    paths = set()
    for k, inst in list(enumerate(many_drops()))[::12]:
        idx = [k % 5]
        g = reduced(inst, ROWS, idx)
        w = ref_drop(ref_state(*inst), ROWS, idx, *g)
        assert w["status"] == oracle.two_phase(*g)["status"]
        paths.add(w["path"])
    assert {"none", "forced+"} <= paths
