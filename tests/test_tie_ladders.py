"""The tie-ladder inputs really are adversarial (CPU, oracle only), so the GPU tests on them
(test_gpu_tie_ladders.py) cannot pass vacuously: on every committed case the combine order of the
eps-argmin tree decides at least the stated number of pivots, on both the entering and the
ratio side, and all k pivots run before the phase ends.  The floors are conditions on the inputs:
a seed that misses one is replaced, the floor is never lowered."""
import numpy as np
import pytest

import oracle
import tie_ladders as tl
from conftest import two_phase_ref


@pytest.mark.parametrize("name", list(tl.CASES))
def test_census_floors(name):
    gen, args, seed, k, enter_floor, ratio_floor = tl.CASES[name]
    A, b, _ = tl.make(name)
    n, m, g = args
    assert A.shape == (m, n) and b.shape == (m,)
    c = tl.census(A, b, k)
    print(name, c)
    assert c["done"] == k
    assert c["enter_sensitive"] >= enter_floor
    assert c["ratio_sensitive"] >= ratio_floor
    # a sensitive pivot has a second value in its winner's window or chain
    assert c["enter_window"] > 0 and c["ratio_window"] > 0


@pytest.mark.parametrize("name", list(tl.TILE_MERGE))
def test_tile_merge_floors(name):
    """the order in which TILE winners are merged (the hand-off between blocks and ranks, not only
    the lanes of one tile) decides at least the case's floor of pivots on the stated side"""
    gen, args, seed, k, enter_floor, ratio_floor = tl.CASES[name]
    A, b, _ = tl.make(name)
    c = tl.tile_merge_census(A, b, k)
    print(name, c)
    side = tl.TILE_MERGE[name]
    assert c["done"] == k
    assert c[side + "_rev"] >= (enter_floor if side == "enter" else ratio_floor)


@pytest.mark.parametrize("name,tiles", [("W64", 64), ("W65", 65), ("W160", 160), ("W161", 161), ("W65x2-1", 65),
                                        ("W65x2-2", 65)])
def test_wide_cases_objective_tiles(name, tiles):
    """N - 1 = n + 2m columns in 512-wide objective tiles: the boundaries of the fused batch's poll
    (64 | 65), its limit (160) and the first width on the per-pivot path (161)"""
    n, m, g = tl.CASES[name][1]
    assert (n + 2 * m + 511) // 512 == tiles
    assert (n + 2 * m) % 512 in (0, 1)
    if name.startswith("W65x2"):
        assert 512 < m <= 1024  # (rows on two 512-aligned shards)


def test_generated_instances_are_not_sensitive():
    """the contrast the ladders exist for: on a generateRandomProblem instance no winner has a
    second, different value inside its eps-window -- the only ties are exact ones (the slack
    columns' -1.0), where the tree picks among equal values -- and no ratio is tree-decided"""
    A, b, c = oracle.generate(200, 1100, 200 * 100 + 1100, 1, 100)
    got = tl.census(A, b, 60)
    assert got["done"] == 60
    assert got["enter_window"] == 0 and got["ratio_window"] == 0 and got["ratio_sensitive"] == 0


def test_eps_scan_and_window():
    e = tl.EPS
    v = np.array([5.0, 5.0 - 0.6 * e, 5.0 - 1.2 * e, 7.0])
    assert int(np.argmin(v)) == 2 and tl.eps_scan(v) == 2  # (1.2 eps below the incumbent: taken)
    v = np.array([5.0, 5.0 - 0.6 * e, 5.0 - 0.9 * e, tl.DBL_MAX])
    assert tl.eps_scan(v) == 0 and int(np.argmin(v)) == 2
    assert tl.window(v, 0).tolist() == [1, 2]
    assert tl.eps_scan(np.array([tl.DBL_MAX, 3.0, tl.DBL_MAX])) == 1


@pytest.mark.parametrize("name", list(tl.WHOLE_SOLVES))
def test_whole_solves_end(name):
    """the ladder LPs the GPU file solves whole (cost vector c = -(1 + q k_j)): the oracle ends both
    phases FEASIBLE, phase 1 within m pivots plus a few hundred (every artificial has to leave)"""
    A, b, _ = tl.make(name)
    m, n = A.shape
    ref = two_phase_ref(A, b, tl.cost_vector(n, 1))
    status, pivots = tl.WHOLE_SOLVES[name]
    assert ref["status"] == status == oracle.FEASIBLE
    assert ref["pivots"] == pivots
    assert m <= pivots[0] <= m + 400 and 0 < pivots[1] <= 400


@pytest.mark.parametrize("L", [4097, 16384, 73728, 100000, 261633, 262144])
def test_ladder_vector_is_tree_decided(L):
    """the second value family of the device argmin test: the oracle's index is not np.argmin's"""
    v = tl.ladder_vector(L)
    i, vm = oracle.argmin(v)
    assert i != int(np.argmin(v)) and vm == v[i]
    assert tl.window(v, i).size > 0


@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_boundary_states_oracle(where):
    """compare()'s eligibility boundaries: an entering-column entry / a reduced cost one ulp below
    1e-9 is not eligible (UNBOUNDED / the phase ends); at 1e-9 and one ulp above, a pivot is taken,
    on that entry"""
    x = tl.BOUNDARY[where]
    assert (np.nextafter(1e-9, 0) < 1e-9 < np.nextafter(1e-9, 1)) and x > 0
    T, d, base = tl.boundary_state("entry", x)
    assert T.shape == (20, 1 + 6 + 40) and T[:, 1 + 3].max() == x
    st, e, r = oracle.pivot(T, d, base)
    assert (st, e) == ((oracle.UNBOUNDED, 3) if where == "below" else (oracle.NOT_ENDED, 3))
    assert r == (-1 if where == "below" else 11)
    T, d, base = tl.boundary_state("cost", x)
    assert d[1:].min() == -x and np.count_nonzero(d[1:] < 0) == 1
    st, e, r = oracle.pivot(T, d, base)
    assert (st, e) == ((oracle.FEASIBLE, 4) if where == "below" else (oracle.NOT_ENDED, 4))


# ------------------------------------------------------------------ the failure message
def _plain_device(T0, d0, base0, wrong_at, side):
    """a stand-in for the device: the oracle, except that at pivot `wrong_at` the entering column
    (or the leaving row) is np.argmin's choice"""
    def run(k):
        T, d, base = T0.copy(), d0.copy(), base0.copy()
        done = 0
        for j in range(k):
            if j != wrong_at:
                assert oracle.pivot(T, d, base)[0] == oracle.NOT_ENDED
            else:
                e, dmin = oracle.argmin(d[1:])
                if side == "enter":
                    e = int(np.argmin(d[1:]))
                    dmin = d[1 + e]
                rv = tl.ratios(T, e)
                r = int(np.argmin(rv)) if side == "ratio" else oracle.argmin(rv)[0]
                base[r] = e
                prow, colE = T[r].copy(), T[:, 1 + e].copy()
                oracle.apply_update(T, d, prow, colE, r, prow[1 + e], dmin)
            done += 1
        return T, d, base, oracle.NOT_ENDED, done
    return run


@pytest.mark.parametrize("side,word", [("enter", "ENTERS"), ("ratio", "LEAVING")])
def test_explain_divergence_names_the_pivot(side, word):
    """explain_divergence on a stand-in device that is wrong at one known tie-sensitive pivot: the
    message names that pivot, the side, and prints the window"""
    A, b, k = tl.make("O-small")
    T0, d0, base0 = tl.phase1_state(A, b)
    T, d, base = T0.copy(), d0.copy(), base0.copy()
    wrong_at = None
    for j in range(k):  # the first pivot np.argmin decides differently on this side
        v = d[1:].copy()
        e = oracle.argmin(v)[0]
        rv = tl.ratios(T, e)
        vec, win = (v, e) if side == "enter" else (rv, oracle.argmin(rv)[0])
        if int(np.argmin(vec)) != win:
            wrong_at = j
            break
        oracle.pivot(T, d, base)
    assert wrong_at is not None
    run = _plain_device(T0, d0, base0, wrong_at, side)
    calls = []

    def run_once(kk):
        calls.append(kk)
        return run(kk)

    got = run(k)
    ref = tl.oracle_trace(T0, d0, base0, k)[3]
    assert not np.array_equal(got[2], ref[2])
    msg = tl.explain_divergence(T0, d0, base0, k, got[2], got[4], run_once)
    assert calls == [wrong_at + 1]  # (one extra device run, with the diverging count)
    assert msg.startswith("first diverging pivot: %d (0-based)" % wrong_at) and word in msg and "eps" in msg


# ------------------------------------------------------------------ whole LPs for the batch kernels
_BATCH = {}


def _batch(name):
    """(A, b, c), the census over both phases and the oracle's result with its objective row of a
    BATCH_CASES case: computed once, never written"""
    if name not in _BATCH:
        A, b, c = tl.make_batch(name)
        ref = oracle.two_phase(A, b, c)
        ref["row"] = oracle.last_objective_row().copy()
        _BATCH[name] = ((A, b, c), tl.census_two_phase(A, b, c), ref)
    return _BATCH[name]


@pytest.mark.parametrize("name", list(tl.BATCH_CASES))
def test_batch_case_floors(name):
    """the whole-LP ladders of test_gpu_batch_ladders.py: the oracle ends FEASIBLE after the stated
    pivots, and in each phase the tree order (B-small: the lanes; the others: the merge of the tile
    winners) decides at least the floor of pivots"""
    gen, (n, m, g), kw, seed, cls, pivots = tl.BATCH_CASES[name]
    (A, b, c), cen, ref = _batch(name)
    print(name, cen)
    assert A.shape == (m, n) and b.shape == (m,) and c.shape == (n,)
    assert (ref["status"], ref["pivots"]) == (oracle.FEASIBLE, pivots) and cen["pivots"] == pivots
    assert len(ref["row"]) == 1 + n + m
    for (phase, key), floor in tl.BATCH_FLOORS[name].items():
        assert cen[phase][key] >= floor, (phase, key)
    if name == "O-small":
        A0, b0, _ = tl.make(name)
        assert np.array_equal(A, A0) and np.array_equal(b, b0) and tl.WHOLE_SOLVES[name] == (oracle.FEASIBLE, pivots)


def test_batch_case_shapes():
    """what each case is sized for: candidates per side in 512-wide tiles, sub-eps trims"""
    shape = {name: tl.BATCH_CASES[name][1][:2] for name in tl.BATCH_CASES}
    n, m = shape["B-small"]
    assert n + 2 * m <= 512  # (one tile on each side in both phases)
    n, m = shape["B-wide3"]
    assert 1024 < n + m and n + 2 * m <= 1536  # (3 entering tiles in both phases)
    n, m = shape["B-w1024"]
    assert n + 2 * m == 1024
    n, m = shape["B-w1025"]
    assert n + 2 * m == 1025
    n, m = shape["B-w65t"]
    assert n + 2 * m == 64 * 512 + 1 and (n + m + 511) // 512 == 64
    n, m = shape["B-ws"]
    assert 512 < m <= 1024 and 1024 < n + 2 * m <= 1536  # (2 ratio tiles, 3 entering tiles in phase 1)
    n, m = shape["B-trim"]
    assert 512 < m <= 1024
    A = tl.make_batch("B-trim")[0]
    assert np.count_nonzero((A > 0) & (A < 1e-9)) > 0


# (ii) merges tile winners, so it is held against the cases with a tile-merge floor; O-small and
# B-small decide inside one tile's lanes (tile_merge_census: 0 on both sides), which (i) covers
_STANDINS = [(name, sel) for name in tl.BATCH_CASES for sel in (tl.select_np, tl.select_tiles_rev)
             if sel is tl.select_np or any(key.endswith("_rev") for _, key in tl.BATCH_FLOORS[name])]


@pytest.mark.parametrize("name,select", _STANDINS, ids=["%s-%s" % (n, s.__name__) for n, s in _STANDINS])
def test_batch_cases_tell_standins_apart(name, select):
    """a whole two-phase solve with another selection rule on both sides -- (i) np.argmin, (ii) the
    reference's tree inside each 512-wide tile with the tile winners merged right to left -- differs
    from the oracle in a field the GPU tests compare (on B-trim only in the bits of the objective
    row and of the objective), so a batch kernel with that rule cannot pass them"""
    (A, b, c), _, ref = _batch(name)
    got = tl.standin_two_phase(A, b, c, select)
    assert not tl.same_result(got, ref)
    if name == "B-trim":
        assert got["pivots"] == ref["pivots"] and np.array_equal(got["base"], ref["base"])
    elif name in ("B-wide3", "B-w1024", "B-w1025", "B-w65t", "B-ws") or select is tl.select_np:
        assert not np.array_equal(got["base"], ref["base"])


def test_standin_with_the_reference_rule_is_the_oracle():
    """the stand-in replay itself is exact: with the oracle's own argmin it returns the oracle's
    result, whole and capped (so a difference above is the selection rule's)"""
    (A, b, c), _, ref = _batch("B-small")
    def rule(v):
        return oracle.argmin(v)[0]
    assert tl.same_result(tl.standin_two_phase(A, b, c, rule), ref)
    for cap in (0, 7, 133, 134, 150):
        want = oracle.two_phase(A, b, c, cap)
        want["row"] = oracle.last_objective_row().copy()
        assert tl.same_result(tl.standin_two_phase(A, b, c, rule, cap), want), cap


@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_boundary_lps_oracle(where):
    """compare()'s eligibility boundaries as whole LPs: phase 1 is m slack pivots that leave the
    tableau as built, and phase 2's first decision is the boundary one"""
    x = tl.BOUNDARY[where]
    for kind in ("entry", "cost"):
        A, b, c = tl.boundary_lp(kind, x)
        m, n = A.shape
        assert (m, n) == (20, 6) and np.all(b > 0) and np.all(b == np.round(b)) and np.all(A.sum(axis=0) < 1)
        T, d, base = tl.phase1_state(A, b)
        T0 = T.copy()
        assert oracle.solve(T, d, base) == (oracle.FEASIBLE, m) and np.array_equal(T, T0)
        assert np.array_equal(base, n + np.arange(m))
    A, b, c = tl.boundary_lp("entry", x)
    assert int(np.argmax(c)) == 3 and A[:, 3].max() == x and np.sort(A[:, 3])[-2] == 0.5e-9
    assert np.signbit(A[7, 3]) and A[7, 3] == 0 and A[15, 3] == tl.BOUNDARY["below"] / 2
    ref = oracle.two_phase(A, b, c)
    if where == "below":
        assert (ref["status"], ref["pivots"]) == (oracle.UNBOUNDED, (20, 0))
    else:
        assert ref["pivots"][0] == 20 and ref["pivots"][1] >= 1 and ref["base"][11] == 3
    A, b, c = tl.boundary_lp("cost", x)
    assert c[4] == x and np.count_nonzero(c > 0) == 1
    ref = oracle.two_phase(A, b, c)
    assert ref["status"] == oracle.FEASIBLE
    assert ref["pivots"] == ((20, 0) if where == "below" else (20, 1))
    assert (4 in ref["base"]) == (where != "below")


@pytest.mark.parametrize("name,select,word", [("B-small", tl.select_np, "ENTERS"), ("B-ws", tl.select_tiles_rev, "LEAVING")])
def test_explain_batch_divergence_names_the_pivot(name, select, word):
    """explain_batch_divergence on a stand-in device: it names a pivot count k at which the stand-in's
    rule really picks differently on the oracle's state after k - 1 pivots, within about 12 runs"""
    (A, b, c), _, ref = _batch(name)
    calls = []

    def run(k):
        calls.append(k)
        got = tl.standin_two_phase(A, b, c, select, max_pivots=k)
        return got["status"], got["pivots"], got["base"]

    msg = tl.explain_batch_divergence(A, b, c, run)
    assert len(calls) <= 13 and all(0 < k <= ref["pivots"][0] for k in calls)
    assert msg.startswith("first differing basis: after %d pivots of phase 1" % calls[-1]) and word in msg and "eps" in msg
    T, d, base = tl.phase1_state(A, b)
    assert oracle.solve(T, d, base, max_pivots=calls[-1] - 1)[1] == calls[-1] - 1
    e = oracle.argmin(d[1:])[0]
    r = oracle.argmin(tl.ratios(T, e))[0]
    assert (select(d[1:]), select(tl.ratios(T, e))) != (e, r)
