"""Every selection path of the engine on tie-ladder tableaux (needs an MI355X).

On the inputs of tests/tie_ladders.py the order of the eps-argmin combine tree decides most pivots
(tests/test_tie_ladders.py holds the floors), so a path that merged lane, tile or rank winners in
another order than the reference's -- linear instead of tree, waves or ranks in another order,
padding handled differently -- ends at another basis.  Bar: T, d, the basis, the pivot count and
the status equal the oracle's bit for bit.  A failure names the first diverging pivot
(tie_ladders.explain_divergence: CPU replay plus one extra device run)."""
import numpy as np
import pytest

import oracle
import simplexoncuda_amd as sx
import tie_ladders as tl
from conftest import two_phase_ref

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


_SETTERS = {"batch": (sx.set_batch, 0), "fused": (sx.set_fused, -1), "p2p": (sx.set_p2p, -1),
            "W": (sx.set_virtual_ranks, 1), "repl": (sx.set_replicated_objective, -1),
            "force": (sx.set_force_exchange, 0), "mode": (sx.set_exchange_mode, 0)}


def _pivots_with(cfg, T, d, base, k):
    Tg, dg, bg = T.copy(), d.copy(), base.copy()
    try:
        for key, val in cfg.items():
            _SETTERS[key][0](val)
        st, done = sx.dev_pivots(Tg, dg, bg, k)
    finally:
        for key in cfg:
            _SETTERS[key][0](_SETTERS[key][1])
    return Tg, dg, bg, st, done


# the initial state of a case and the oracle's state after its k pivots: computed once, never
# written (the small cases are kept; of the wide ones, the one in use)
_SMALL, _WIDE = {}, {}


def _case(name):
    cache = _WIDE if name.startswith("W") else _SMALL
    if name not in cache:
        _WIDE.clear()
        A, b, k = tl.make(name)
        T0, d0, base0 = tl.phase1_state(A, b)
        T, d, base = T0.copy(), d0.copy(), base0.copy()
        st, done = oracle.solve(T, d, base, max_pivots=k)
        assert st == oracle.PIVOT_CAP and done == k  # (no phase end inside the k pivots)
        cache[name] = (T0, d0, base0, k, (T, d, base))
    return cache[name]


def _check(name, cfg, fused=None):
    """the case through sx.dev_pivots under cfg against the oracle; fused: True / False = the
    engine's fused-batch counter must / must not advance (and no hand-off may time out)"""
    T0, d0, base0, k, (T, d, base) = _case(name)
    lib = sx.load()
    f0, h0 = lib.simplex_fused_batches(), lib.simplex_hang_recoveries()
    Tg, dg, bg, st, done = _pivots_with(cfg, T0, d0, base0, k)
    f1, h1 = lib.simplex_fused_batches(), lib.simplex_hang_recoveries()
    if not (done == k and st == sx.NOT_ENDED and np.array_equal(bg, base) and same(dg, d) and same(Tg, T)):
        why = tl.explain_divergence(T0, d0, base0, k, bg, done, lambda kk: _pivots_with(cfg, T0, d0, base0, kk))
        pytest.fail("%s under %r: status %d, %d of %d pivots, basis %s, d %s, T %s -- %s" % (
            name, cfg, st, done, k, "equal" if np.array_equal(bg, base) else "DIFFERS",
            "equal" if same(dg, d) else "DIFFERS", "equal" if same(Tg, T) else "DIFFERS", why))
    assert h1 == h0
    if fused is not None:
        assert (f1 > f0) == fused, "fused batches %d -> %d under %r" % (f0, f1, cfg)


# ------------------------------------------------------------------ D, O, O-small: every path
_CFGS = [("fused-b1", {"batch": 1}, True), ("fused-b32", {"batch": 32}, True), ("fused-b64", {"batch": 64}, True),
         ("per-pivot", {"fused": 0}, False)]
_CFGS += [("p2p-W%d-b%d-repl%d" % (W, batch, repl), {"W": W, "p2p": 1, "batch": batch, "repl": repl}, True)
          for W in (2, 3, 8) for batch in (32, 64) for repl in (0, 1)]
# the exchange path: mode 1 selects with k_select_row, mode 2 with k_select_gathered
_CFGS += [("exchange-W%d-mode%d" % (W, mode), {"W": W, "force": 1, "mode": mode}, False)
          for W in (2, 3, 1) for mode in (1, 2)]


@pytest.mark.parametrize("cfg", _CFGS, ids=[c[0] for c in _CFGS])
@pytest.mark.parametrize("name", ["D-1", "D-2", "O-1", "O-2", "O-small", "O-tiles-1", "O-tiles-2"])
def test_ladder_pivots_every_path(gpu, name, cfg):
    """k pivots of a ladder tableau: one shard's fused batch (one pivot per batch, one stage, two
    stages), the per-pivot path (k_ratio_select's last-block pass, k_pivot_row), the multi-rank
    fused batch on 2, 3 and 8 virtual shards with the objective tiles split or replicated, and both
    exchange paths on 1-3 shards.  D and O decide their ratios across row tiles and shards, O-tiles
    its entering columns across objective tiles and ranks (tie_ladders.TILE_MERGE)"""
    _check(name, cfg[1], cfg[2])


# ------------------------------------------------------------------ objective-tile boundaries
@pytest.mark.parametrize("batch", [0, 64])
@pytest.mark.parametrize("name", ["W64", "W65", "W160"])
def test_wide_ladders_fused(gpu, name, batch):
    """64, 65 and 160 objective tiles on one shard (the widths at which the fused batch's poll of
    the tile records changes, and its limit): default and 64-pivot batches, every batch fused"""
    _check(name, {"batch": batch}, True)


def test_wide_ladder_past_fused_limit(gpu):
    """161 objective tiles: one more than the fused batch holds (sx_batch_fits, Engine::fused_ok),
    so the engine runs the per-pivot path -- no fused batch -- and stays bit-exact"""
    n, m, _ = tl.CASES["W161"][1]
    assert (n + 2 * m + 511) // 512 == 161
    _check("W161", {}, False)


@pytest.mark.parametrize("cfg", [{"W": 2, "p2p": 1, "repl": 0}, {"W": 2, "p2p": 1, "repl": 1},
                                 {"W": 2, "force": 1, "mode": 2}], ids=["p2p-repl0", "p2p-repl1", "exchange-mode2"])
@pytest.mark.parametrize("name", ["W65x2-1", "W65x2-2"])
def test_wide_ladders_two_shards(gpu, name, cfg):
    """65 objective tiles with the rows on two 512-aligned shards: the multi-rank fused batch
    (tiles split 33 + 32, or all 65 on both ranks) and the row-gather exchange"""
    _check(name, cfg, "p2p" in cfg)


# ------------------------------------------------------------------ whole solves
@pytest.mark.parametrize("batch", [0, 64])
@pytest.mark.parametrize("name", list(tl.WHOLE_SOLVES))
def test_ladder_two_phase(gpu, name, batch):
    """whole two-phase solves of ladder LPs (cost vector c = -(1 + q k_j)): the phase switch, the
    GEMV and the phase-2 restart on ladder data; every bit of the answer vs the oracle"""
    A, b, _ = tl.make(name)
    c = tl.cost_vector(A.shape[1], 1)
    ref = two_phase_ref(A, b, c)
    assert (ref["status"], ref["pivots"]) == tl.WHOLE_SOLVES[name]
    p = sx.Problem.from_arrays(A, b, c)
    try:
        sx.set_batch(batch)
        got = sx.twoPhaseMethodEx(p)
    finally:
        sx.set_batch(0)
    assert got.status == ref["status"] == sx.FEASIBLE
    assert tuple(got.pivots) == ref["pivots"]
    assert np.array_equal(got.base, ref["base"])
    assert same(got.optimal_value, ref["opt"])
    assert same(got.solution, ref["x"])


# ------------------------------------------------------------------ compare()'s eligibility boundaries
@pytest.mark.parametrize("fused", [-1, 0])
@pytest.mark.parametrize("where", ["below", "at", "above"])
@pytest.mark.parametrize("kind", ["entry", "cost"])
def test_eligibility_boundary(gpu, kind, where, fused):
    """one pivot of a hand-built 20 x 47 state whose entering column's largest entry ("entry") or
    whose most negative reduced cost ("cost") is one ulp below 1e-9, 1e-9, one ulp above: not
    eligible below (UNBOUNDED / the phase ends), a pivot on that entry otherwise -- the oracle's
    status and bits, on the fused batch and on the per-pivot path"""
    T, d, base = tl.boundary_state(kind, tl.BOUNDARY[where])
    Tg, dg, bg, st, done = _pivots_with({"fused": fused}, T, d, base, 1)
    st_o, done_o = oracle.solve(T, d, base, max_pivots=1)
    if where == "below":
        assert st_o == (oracle.UNBOUNDED if kind == "entry" else oracle.FEASIBLE) and done_o == 0
        assert st == st_o
    else:
        assert st_o == oracle.PIVOT_CAP and done_o == 1
        assert st == sx.NOT_ENDED
        assert base[base < 26].tolist() == [3 if kind == "entry" else 4]  # (the one structural column in the basis)
    assert done == done_o
    assert np.array_equal(bg, base) and same(dg, d) and same(Tg, T)
