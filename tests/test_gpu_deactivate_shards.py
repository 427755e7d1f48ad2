"""Basic slack columns moved out of the sweep on the row-block shards of one process (DESIGN.md
§3.4; k_deact_* in sx_kernels.hip, Engine::enqueue_sweep).

Each shard checks only its rows of a listed column, and every shard plans from the OR of all the
shards' verdicts, so the slack permutation stays replicated.  Every logical entry of the tableau must
stay the CPU oracle's bit for bit; the swept slack count must be the same on every shard and equal to
a one-shard session's under the same batch size and cadence (the swept set is a function of the pivot
history and the round schedule only), and below the count without deactivation (needs an MI355X).
"""
import numpy as np
import pytest

import simplexoncuda_amd as sx
from conftest import two_phase_ref
from test_deactivate_shards_fixture import block_diag_instance, oracle_checkpoints

pytestmark = pytest.mark.gpu

_ONE_SHARD = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(autouse=True)
def _no_hang_recovery():
    lib = sx.load()
    h0 = lib.simplex_hang_recoveries()
    yield
    assert lib.simplex_hang_recoveries() == h0


def _reset():
    sx.set_gpus([])
    sx.set_virtual_ranks(1)
    sx.set_p2p(-1)
    sx.set_batch(0)
    sx.set_deactivate(sx.DEACTIVATE_EVERY)
    sx.set_deactivate_shards(1)
    sx.set_replicated_objective(-1)
    sx.set_mr_single_launch(1)


def _session_run(p, stops, W, p2p, deact, batch, shards=1, gpus=False):
    """(batch size in use, [(status, pivots, T, d, base, per-shard swept slack counts)] per stop);
    gpus: the W shards as a device list on this GPU instead of virtual ranks"""
    out = []
    try:
        if gpus:
            sx.set_gpus([0] * W)
        else:
            sx.set_virtual_ranks(W)
        sx.set_p2p(p2p)
        sx.set_deactivate(deact)
        sx.set_deactivate_shards(shards)
        sx.set_batch(batch)
        s = sx.Session(problem=p)
        K = s.batch()
        for k in stops:
            t = s.pivots(k - s.total_pivots())
            Tg, dg, bg = s.tableau(p.m, 1 + p.n + 2 * p.m)
            counts = s.shard_active_slacks()
            assert len(counts) == W and s.active_slacks() == counts[0]
            out.append((t.status, s.total_pivots(), Tg, dg, bg, counts))
            if t.status != sx.NOT_ENDED:
                break
        s.close()
    finally:
        _reset()
    return K, out


def _one_shard_counts(name, p, stops, deact, K):
    """a one-shard session's swept slack count at each stop (batch size K), computed once"""
    key = (name, tuple(stops), deact, K)
    if key not in _ONE_SHARD:
        K1, run = _session_run(p, stops, 1, -1, deact, K)
        assert K1 == K
        _ONE_SHARD[key] = [r[5][0] for r in run]
    return _ONE_SHARD[key]


def _check_against_oracle(name, p, stops, W, p2p, every, batch, gpus=False):
    A, b, c = p.arrays()
    K, on = _session_run(p, stops, W, p2p, every, batch, gpus=gpus)
    ref = oracle_checkpoints(A, b, stops)
    one = _one_shard_counts(name, p, stops, every, K)
    off = _one_shard_counts(name, p, stops, 0, K)
    assert len(on) == len(stops)
    moved_out = False
    for (st, k, T1, d1, b1, counts), (T, d, base, done), a1, a0 in zip(on, ref, one, off):
        print(name, "W", W, "p2p", p2p, "every", every, "batch", K, "pivots", k, "swept", counts, "one shard", a1,
              "without", a0)
        assert k == done and st == sx.NOT_ENDED
        assert same(T1, T) and same(d1, d) and np.array_equal(b1, base), k
        assert counts == [counts[0]] * W, k  # (the shards agree)
        assert counts[0] == a1, k            # (and with one shard)
        assert a1 <= a0
        moved_out = moved_out or counts[0] < a0
    assert moved_out  # (basic slacks did leave the sweep: fails while only one shard deactivates)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("p2p", [1, 0])  # peer-memory batches / the per-pivot exchange
@pytest.mark.parametrize("W", [2, 3, 8])  # (8: shards without rows)
@pytest.mark.parametrize("n,m,seed,stops,batch", [
    (64, 700, 7107, (150, 400, 700), 0),
    (16, 1536, 3143, (500, 1200), 64),  # few structurals: the slacks re-enter quickly
])
def test_shards_tableau_bit_exact(gpu, n, m, seed, stops, batch, W, p2p, every):
    p = sx.generateRandomProblem(n, m, seed, 1, 100)
    _check_against_oracle("%dx%d" % (n, m), p, stops, W, p2p, every, batch)


def _whole_solve(p):
    got = sx.twoPhaseMethodEx(p)
    A, b, c = p.arrays()
    ref = two_phase_ref(A, b, c)
    assert got.status == ref["status"] and tuple(got.pivots) == ref["pivots"]
    assert np.array_equal(got.base, ref["base"])
    if got.status == sx.FEASIBLE:
        assert same(got.optimal_value, ref["opt"]) and same(got.solution, ref["x"])
    return got


@pytest.mark.parametrize("p2p", [1, 0])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_shards_that_disagree(gpu, W, p2p):
    """blockdiag(A1, A2), rows [0, 512) and [512, 1212): basic slack columns with residuals in one
    block only (tests/test_deactivate_shards_fixture.py), so at W = 3 (rows per shard 512) and W = 2
    (1024) some shard with rows sees an exact part of e_r where another sees residuals.  Planning
    from a shard's own verdict, from shard 0's or from none breaks the tableau or the agreement."""
    p = sx.Problem.from_arrays(*block_diag_instance())
    _check_against_oracle("blockdiag", p, (200, 600, 1300), W, p2p, 1, 0)
    try:
        sx.set_virtual_ranks(W)
        sx.set_p2p(p2p)
        sx.set_deactivate(1)
        got = _whole_solve(p)
    finally:
        _reset()
    assert got.status == sx.FEASIBLE and tuple(got.pivots) == (1531, 69)


@pytest.mark.parametrize("deact", [1, 8])
@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("n,m,seed,lo", [
    (300, 1100, 41100, 1), (64, 128, 6528, 1),
    (129, 1513, 77, -100),  # negated rows: no slack compaction, the path must be inert
])
def test_shards_two_phase(gpu, n, m, seed, lo, W, deact):
    p = sx.generateRandomProblem(n, m, seed, lo, 100)
    try:
        sx.set_virtual_ranks(W)
        sx.set_p2p(1)
        sx.set_deactivate(deact)
        _whole_solve(p)
    finally:
        _reset()


@pytest.mark.parametrize("p2p", [-1, 0])  # the list's self-check decides (peer-memory batches) / per-pivot exchange
def test_device_list_tableau_bit_exact(gpu, p2p):
    """the device-list form of the shards (every shard on this GPU), on the instance whose shards disagree"""
    p = sx.Problem.from_arrays(*block_diag_instance())
    _check_against_oracle("blockdiag", p, (200, 600, 1300), 3, p2p, 1, 0, gpus=True)


@pytest.mark.parametrize("variant", ["replicated_objective", "launch_per_rank", "batch64", "device_list",
                                     "device_list_exchange"])
def test_shards_two_phase_variants(gpu, variant):
    p = sx.generateRandomProblem(300, 1100, 41100, 1, 100)
    lib = sx.load()
    f0 = lib.simplex_fused_batches()
    try:
        sx.set_p2p(1)
        if variant.startswith("device_list"):
            sx.set_p2p(-1 if variant == "device_list" else 0)  # (-1: the list's own start-up self-check decides)
            sx.set_gpus([0, 0])
        else:
            sx.set_virtual_ranks(2)
        if variant == "replicated_objective":
            sx.set_replicated_objective(1)
        if variant == "launch_per_rank":
            sx.set_mr_single_launch(0)
        if variant == "batch64":
            sx.set_batch(64)
        sx.set_deactivate(1)
        _whole_solve(p)
        if variant == "device_list":  # (its self-check passed: the batches ran on the peer-memory path)
            assert lib.simplex_p2p_ready() == 1 and lib.simplex_fused_batches() > f0
    finally:
        _reset()


def test_shards_switch_off(gpu):
    """simplex_set_deactivate_shards(0): the one-shard-only rule, the counts of no deactivation"""
    p = sx.generateRandomProblem(64, 700, 7107, 1, 100)
    stops = (150, 400, 700)
    K, held = _session_run(p, stops, 2, 1, 1, 0, shards=0)
    K0, off = _session_run(p, stops, 2, 1, 0, 0)
    K1, on = _session_run(p, stops, 2, 1, 1, 0)
    assert K == K0 == K1
    assert [r[5] for r in held] == [r[5] for r in off]
    assert any(a[5][0] < b[5][0] for a, b in zip(on, off))
    ref = oracle_checkpoints(*p.arrays()[:2], stops)
    for (st, k, T1, d1, b1, _), (T, d, base, done) in zip(held, ref):
        assert k == done and same(T1, T) and same(d1, d) and np.array_equal(b1, base)
