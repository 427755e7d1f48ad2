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
