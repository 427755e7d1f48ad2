"""The block-diagonal instance behind tests/test_gpu_deactivate_shards.py (CPU oracle only).

Row-block shards combine their per-shard checks before a basic slack column leaves the sweep
(DESIGN.md §3.4).  On a random instance a densely re-entered column keeps residuals in nearly every
row, so every shard fails it and the combination is never exercised.  A = blockdiag(A1, A2) keeps
each slack column an exact +0 outside its own block: a column with residuals is failed by the
shards holding its block and passed -- an exact e_r part, or all +0 -- by the others.  This file
pins that precondition, so the GPU test cannot quietly cease to test the combination.
"""
import numpy as np

import oracle

SPLIT = 512  # rows of the first block: a shard boundary at W = 3 (rows per shard 512), inside shard 0 at W = 2
_CHECKPOINTS = {}


def block_diag_instance():
    """(A, b, c): n = 128, m = 1212, blocks (64 x 512, seed 6919) and (64 x 700, seed 7107)"""
    A1, b1, c1 = oracle.generate(64, 512, 6919, 1, 100)
    A2, b2, c2 = oracle.generate(64, 700, 7107, 1, 100)
    A = np.zeros((A1.shape[0] + A2.shape[0], A1.shape[1] + A2.shape[1]))
    A[:A1.shape[0], :A1.shape[1]] = A1
    A[A1.shape[0]:, A1.shape[1]:] = A2
    return A, np.concatenate([b1, b2]), np.concatenate([c1, c2])


def oracle_checkpoints(A, b, stops):
    """[(T, d, base, pivots done)] of the oracle's phase 1 at each stop (computed once per instance
    and stop list; callers must not modify the arrays)"""
    key = (A.tobytes(), b.tobytes(), tuple(stops))
    if key not in _CHECKPOINTS:
        T, d, base = oracle.build_phase1(A, b)
        oracle.update_objective(T, d, base)
        out, done = [], 0
        for k in stops:
            _, step = oracle.solve(T, d, base, max_pivots=k - done)
            done += step
            out.append((T.copy(), d.copy(), base.copy(), done))
        _CHECKPOINTS[key] = out
    return _CHECKPOINTS[key]


def one_sided_basic_slacks(T, base, n, m):
    """basic slack columns that differ from their unit vector, bit for bit, only in rows < SPLIT /
    only in rows >= SPLIT: two lists of (unit row, slack)"""
    low, high = [], []
    for r in range(m):
        k = int(base[r]) - n
        if k >= m:
            k -= m  # (a phase-1 artificial: bit-identical to its slack column, stored as it)
        if k < 0 or k >= m:
            continue
        e = np.zeros(m)
        e[r] = 1.0
        rows = np.nonzero(T[:, 1 + n + k].view(np.uint64) != e.view(np.uint64))[0]
        if rows.size and rows.max() < SPLIT:
            low.append((r, k))
        elif rows.size and rows.min() >= SPLIT:
            high.append((r, k))
    return low, high


def test_block_diagonal_instance_makes_shards_disagree():
    A, b, c = block_diag_instance()
    m, n = A.shape
    assert (n, m) == (128, 1212) and b.shape == (m,) and c.shape == (n,)
    T, d, base, done = oracle_checkpoints(A, b, (200,))[0]
    assert done == 200
    low, high = one_sided_basic_slacks(T, base, n, m)
    print("residuals only in rows < 512:", low, "only in rows >= 512:", high)
    assert len(low) >= 1 and len(high) >= 1
