"""The inputs of tests/test_gpu_dual_ladders.py decide what that file claims (CPU only: the oracle and
the restatements of the kept-state entries).

For every committed case of tests/dual_ladders.py: the kept state is what the construction says; at the
pinned decision the eps-argmin tree's pick differs from np.argmin's, from a left-to-right eps-scan's and,
over more than one 512-wide tile, from the tile winners merged right to left; and the restatement with
np.argmin (with the reversed tile merge) at that one site differs from the true restatement under
dual_ladders.same_result, the comparison of the GPU file's fields -- so a kernel with that rule at that
site cannot pass there.  The floors and the census table of the module's docstring are what this file
measures."""
from functools import partial

import numpy as np
import pytest

import dual_ladders as dl
import oracle
import simplexoncuda_amd as sx
import tie_ladders as tl
from batch_rhs_refs import first_min, ref_rhs_resume

PINS = dl.pins()


def _differs(want, site, **kw):
    """every stand-in at `site` gives another result than the tree; the names of the stand-ins tried"""
    true = want(**kw)
    assert dl.same_result(true, true) and dl.passes_the_gpu_comparison(true, true)
    res = dl.standin_results(want, site, **kw)
    for name, r in res.items():
        assert not dl.same_result(r, true), name
        assert not dl.passes_the_gpu_comparison(r, true), name  # the GPU file's own comparison
    return set(res)


# ------------------------------------------------------------------ (a): the dual loop
@pytest.mark.parametrize("name", list(dl.ORIGIN))
def test_origin_state_is_the_raw_tableau(name):
    (n, m, groups, g), _, cls, _, _ = dl.ORIGIN[name]
    assert sx.batch_class(n, m) == cls
    for k in range(dl.neighbours(cls)):
        case = dl.origin_case(name, dl.ORIGIN[name][1] + k)
        assert dl.is_raw(case["state"], case["A"], case["b"], case["c"])
        A = case["A"]
        for t, r in enumerate(case["rows"]):
            assert np.array_equal(np.flatnonzero(A[r]), case["cols"][t]) and (A[r, case["cols"][t]] == -1.0).all()
            assert np.count_nonzero(A[:, case["cols"][t]]) == g
        neg = case["b2"] < 0
        assert np.array_equal(np.flatnonzero(neg), case["rows"]) and np.array_equal(case["b2"][~neg], case["b"][~neg])


@pytest.mark.parametrize("name", list(dl.ORIGIN))
def test_origin_dual_loop_floors(name):
    """`groups` dual pivots (or a few more), FEASIBLE; the tree decides at least the floor of them on
    either side; np.argmin -- and the reversed tile merge where a side has tiles -- at that side alone
    ends somewhere else"""
    (n, m, groups, g), _, cls, enter_floor, leave_floor = dl.ORIGIN[name]
    want = partial(dl.want_rhs, dl.origin_case(name))
    true = want()
    assert true["status"] == oracle.FEASIBLE and true["dual"] >= groups and true["pivots"][0] == m
    enter, leave = dl.recorded(want, "enter_argmin"), dl.recorded(want, "leave_argmin")
    assert len(enter) == true["dual"] and all(p["len"] == n + m for p in enter)
    assert len(leave) == true["dual"] + 1 and all(p["len"] == m for p in leave)
    assert sum(map(dl.decided, enter)) >= enter_floor
    assert sum(map(dl.decided, leave[:-1])) >= leave_floor  # (the last selection finds no negative row)
    assert enter_floor or leave_floor
    if enter_floor:
        assert _differs(want, "enter_argmin") == ({"np.argmin"} if n + m <= 512 else set(dl.STANDINS))
    if leave_floor:
        assert _differs(want, "leave_argmin") == ({"np.argmin"} if m <= 512 else set(dl.STANDINS))
    # both sides at once: batch_rhs_refs.first_min, the stand-in of test_batch_rhs_host.py
    assert not dl.same_result(want(argmin=first_min), true)


@pytest.mark.parametrize("name", list(dl.ORIGIN))
@pytest.mark.parametrize("cap", [1, 2])
def test_origin_caps_stop_inside_the_dual_loop(name, cap):
    """a cap of 1 and 2 leaves a phase-3 state after that many tree-decided pivots, and its plain resume
    is the uncapped re-solve"""
    case = dl.origin_case(name)
    capped = dl.want_rhs(case, cap)
    assert (capped["status"], capped["phase"], capped["pivots"][1]) == (oracle.PIVOT_CAP, 3, cap)
    assert dl.same_result(ref_rhs_resume(capped, case["c"]), dl.want_rhs(case))


# ------------------------------------------------------------------ single pinned decisions
@pytest.mark.parametrize("pin", PINS, ids=[p[0] for p in PINS])
def test_pinned_decision(pin):
    name, site, key, want, count, (n, m), cls = pin
    assert sx.batch_class(n, m) == cls
    seen = dl.recorded(want, key)
    assert len(seen) >= count
    for p in seen[:count]:
        assert dl.decided(p), p
        assert p["window"] >= 8, p
    tiles = any(p["len"] > 512 for p in seen[:count])
    assert _differs(want, key) == (set(dl.STANDINS) if tiles else {"np.argmin"})
    true = want()
    true = true[3] if isinstance(true, tuple) else true
    assert true["status"] == oracle.FEASIBLE


def test_every_site_has_its_shapes():
    """both classes and one, two and three candidate tiles at the dual entering site; one and two row
    tiles at the leaving, forced-ratio and cut-row sites"""
    enter = {(cls, -(-(n + m) // 512)) for (n, m, _, _), _, cls, fe, _ in dl.ORIGIN.values() if fe}
    assert {t for _, t in enter} == {1, 2, 3} and {c for c, _ in enter} == {1, 2}
    leave = {-(-m // 512) for (_, m, _, _), _, _, _, fl in dl.ORIGIN.values() if fl}
    assert leave == {1, 2}
    for site in ("forced+", "forced-", "cut-row"):
        rows = {-(-dl.recorded(p[3], p[2])[0]["len"] // 512) for p in PINS if p[1] == site}
        assert rows == {1, 2}, site
    dual = {-(-dl.recorded(p[3], p[2])[0]["len"] // 512) for p in PINS if p[1] == "forced-dual"}
    assert dual == {1, 2, 3}
    assert {p[1] for p in PINS} | {"dual-leave"} == set(dl.SITES)


# ------------------------------------------------------------------ the constructions' states
@pytest.mark.parametrize("name", list(dl.SECOND))
def test_second_step_state(name):
    """K1: x_e basic in row r_0 at 1 + 2 q k', +1.0 on the rest of group 0, every d_j there within eps of 0"""
    a = dl.SECOND[name][0]
    kc = dl.second_case(name)
    case = dl.origin_case(a, dl.SECOND[name][1])
    K, r0, e = kc["state"], kc["row"], kc["e"]
    n = case["A"].shape[1]
    assert (K["status"], K["phase"], K["dual"]) == (oracle.FEASIBLE, 2, 1)
    rest = np.setdiff1d(case["cols"][0], [e])
    assert e in case["cols"][0] and K["T"][r0, 0] == -kc["b"][r0] > 0
    assert (K["T"][r0, 1 + rest] == 1.0).all() and K["T"][r0, 1 + e] == 1.0 and K["T"][r0, 1 + n + r0] == -1.0
    assert (np.abs(K["d"][1 + rest]) < 2 * dl.EPS).all() and K["d"][1 + e] == 0.0
    drop, child = dl.want_drop_col(kc), [dl.want_child(kc, k) for k in (0, 1)]
    assert (drop["path"], drop["status"]) == ("forced-dual", oracle.FEASIBLE)
    assert [c["dual"] for c in child] == [1, 1]
    # the drop's excluded candidate would win: its own column has the ratio 0 / 1
    assert K["d"][1 + e] / K["T"][r0, 1 + e] < min(K["d"][1 + rest]) + dl.EPS


@pytest.mark.parametrize("name", list(dl.MINUS))
def test_minus_state(name):
    """a phase-3 state in which x_e's row has a negative right-hand side and -1.0 on group 0"""
    mc = dl.minus_case(name)
    K, p, e = mc["state"], mc["row"], mc["e"]
    assert (K["status"], K["phase"], K["pivots"][1]) == (oracle.PIVOT_CAP, 3, 1)
    assert K["base"][p] == e and K["T"][p, 0] == -0.25 and K["T"][p, 1 + e] == 1.0
    assert np.count_nonzero(K["T"][p, 1:1 + K["T"].shape[1] - 1 - K["T"].shape[0]] == -1.0) == dl.MINUS[name][0][2]
    w = dl.want_drop_col(mc)
    assert (w["path"], w["why"], w["status"]) == ("forced-dual", None, oracle.FEASIBLE)


@pytest.mark.parametrize("name", list(dl.CHAIN))
def test_chain_state(name):
    """x is the ladder, every chain variable basic, and the dropped row's slack nonbasic with +-1.0 in all
    L rows of the chain variables and nothing of that sign elsewhere"""
    (L, m, sign), _, _ = dl.CHAIN[name]
    cc = dl.chain_case(name)
    st = cc["state"]
    assert st["status"] == oracle.FEASIBLE and st["phase"] == 2
    assert np.abs(st["x"][:L] - (1.0 + dl.Q * cc["k"])).max() < 1e-12 and st["x"][L] == 0.0
    col = st["T"][:, 1 + (L + 1) + int(cc["pos"][0])]
    rows = np.flatnonzero(st["base"] < L)
    assert len(rows) == L and not (st["base"] == L + 1 + cc["pos"][0]).any()
    assert (np.abs(col[rows] - sign) < 1e-12).all() and not (sign * np.delete(col, rows) >= dl.EPS).any()
    w = dl.want_drop_rows(cc)
    assert w["paths"] == ["forced+" if sign > 0 else "forced-"]


def test_chain_second_drop_runs_on_the_shrunk_tableau():
    w = dl.want_drop_rows(dl.chain_case("C+24", q=2))
    assert w["paths"] == ["forced+", "forced+"] and w["forced"] == 2 and w["status"] == oracle.FEASIBLE
    seen = dl.recorded(partial(dl.want_drop_rows, dl.chain_case("C+24", q=2)), "argmin")
    assert [p["len"] for p in seen] == [27, 26]


@pytest.mark.parametrize("name", list(dl.BOX))
def test_box_state(name):
    """x_j is basic in its own row at 3.5 + q k_j: all L box rows are eligible, with the keys -(1/2 - q k_j)"""
    from batch_cut_refs import AWAY, row_keys

    (L, m), _, _ = dl.BOX[name]
    xc = dl.box_case(name)
    st = xc["state"]
    assert st["status"] == oracle.FEASIBLE and np.array_equal(st["base"][xc["pos"]], np.arange(L))
    assert np.abs(st["T"][xc["pos"], 0] - (3.5 + dl.Q * xc["k"])).max() < 1e-14  # (q = 1.25e-10)
    keys = row_keys(st, np.ones(L + 2, dtype=bool), AWAY)
    assert np.array_equal(np.flatnonzero(keys != tl.DBL_MAX), xc["pos"])
    assert np.abs(keys[xc["pos"]] + (0.5 - dl.Q * xc["k"])).max() < 1e-14
    three = dl.want_cut(xc, 3)
    assert len(set(three[2].tolist())) == 3 and (three[2] >= 0).all() and three[3]["status"] == oracle.FEASIBLE
    # the marks move the ladder: cut t's row is the tree's pick with the rows already taken left out
    taken = []
    for t in range(3):
        assert three[2][t] == oracle.argmin(row_keys(st, np.ones(L + 2, dtype=bool), AWAY, taken))[0]
        taken.append(int(three[2][t]))
    assert dl.want_cut(xc, 1)[2][0] == three[2][0]
