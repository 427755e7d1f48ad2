#!/usr/bin/env python3
"""Branching a kept batch state on the device against what a caller had to do without the entry.

For each shape (32x16 and 64x64: n variables x m constraints, values in [1,100]) 1024 generated
parents are solved once with keep_state=True.  Every parent gets two children through the largest
component x*_j of its kept optimum, down (x_j <= floor(x*_j)) and up (-x_j <= -(floor(x*_j) + 1)):
C = 2048.  Three paths to the children take turns inside every repeat, each call followed by
torch.cuda.synchronize() under one host clock:

  (a) branch    sx.branch_batch_tensors on the parents' state and the root tensors;
  (b) gather    what a caller does without it: index_select of the five state tensors, the explicit
                A, b and c of every child made with index_select and torch.cat, then
                sx.add_rows_batch_tensors -- all of it inside the timed call, since all of it is
                repeated on every level of a tree;
  (c) scratch   sx.solve_batch_tensors on the explicit children (made once, outside the clock).

(a) and (b) are asserted equal bit for bit, state included, and (c) to end in the same statuses.  The
strong-branching row probes 8 candidates per parent (the 8 largest components, down) for at most two
dual pivots, through (a) with keep_state=False and through (b) with max_pivots=2, which cannot help
keeping the state.  Printed per path: the median, the minimum and the maximum of the repeats, and the
bytes the path moves through device memory per call for warm children, counted from the shapes
(bytes_moved below).  Written to profiles/branch_bench.txt (or --out).

    python scripts/branch_bench.py [--parents 1024] [--repeats 21] [--warmup 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import simplexoncuda_amd as sx  # noqa: E402

SHAPES = [(32, 16), (64, 64)]
STATE_FIELDS = ("T", "d", "base", "phase", "pivots")


def seconds_in_turn(fns, repeats):
    """every time of several functions timed one after the other inside every repeat"""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for ts, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return times


def device_tensors(probs):
    """A [B, m, n], b [B, m], c [B, n] of the problems, on the GPU"""
    arrays = [p.arrays() for p in probs]
    return tuple(torch.from_numpy(np.stack([a[k] for a in arrays])).cuda() for k in range(3))


def state_bytes(n, m):
    """one problem of a BatchState"""
    return 8 * (m * (1 + n + m) + (1 + n + 2 * m)) + 4 * m + 4 + 16


def bytes_moved(n, m0, C, keep_state, objective_row):
    """(branch, gather): device-memory bytes per call, reads plus writes, of C warm children of shape
    (n, m0 + 1) with q = 1.  Both kernels read the parent's state and write the results; the branch kernel
    reads five numbers per child (parent, root, variable, coefficient, right-hand side) and writes the
    out-state only with keep_state; the rows kernel reads the new row's n + 1 entries and always writes
    the out-state, and in front of it the gather path reads and writes a copy of every parent's state
    and reads the root's A, b, c to write the explicit child's"""
    m = m0 + 1
    results = 4 + 16 + 8 + 8 * n + 4 * m + ((8 * (1 + n + 2 * m) + 4) if objective_row else 0)
    branch = C * (state_bytes(n, m0) + results + (state_bytes(n, m) if keep_state else 0) + 4 + 4 + 4 + 8 + 8)
    copies = 2 * state_bytes(n, m0) + 8 * ((m0 * n + m * n) + (m0 + m) + 2 * n)
    gather = C * (state_bytes(n, m0) + results + state_bytes(n, m) + 8 * (n + 1) + copies)
    return branch, gather


def gather_path(state, parent64, var64, coef, rhs, A, b, c, **kw):
    """a caller without the branch entry: copies of the state, the explicit problem, add_rows"""
    gathered = sx.BatchState(*(getattr(state, f).index_select(0, parent64) for f in STATE_FIELDS), state.n, state.m,
                             state.rhs)
    row = torch.zeros((parent64.shape[0], 1, A.shape[2]), dtype=torch.float64, device=A.device)
    row.scatter_(2, var64[:, :, None], coef[:, :, None])
    A2 = torch.cat([A.index_select(0, parent64), row], dim=1)
    b2 = torch.cat([b.index_select(0, parent64), rhs], dim=1)
    return sx.add_rows_batch_tensors(gathered, A2, b2, c.index_select(0, parent64), **kw), (A2, b2)


def same(x, y, state=True):
    for f in ("status", "pivots", "base"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f
    for f in ("optimal_value", "solution"):
        assert torch.equal(getattr(x, f).view(torch.int64), getattr(y, f).view(torch.int64)), f
    if state:
        for f in ("base", "phase", "pivots"):
            assert torch.equal(getattr(x.state, f), getattr(y.state, f)), f
        for f in ("T", "d"):
            assert torch.equal(getattr(x.state, f).view(torch.int64), getattr(y.state, f).view(torch.int64)), f


def timed(fn):
    def run():
        fn()
        torch.cuda.synchronize()
    return run


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:.3f} {min(ts) * 1e3:.3f} {max(ts) * 1e3:.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parents", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("branch_bench.py measures on a GPU; none is available")
    torch.cuda.set_device(0)
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.parents} parents, {args.warmup} warm-up and {args.repeats} timed "
             "repeats per path, in turn; times in ms as median min max; MB per call counted from the shapes",
             "# two children: n m0 children | branch_ms | gather_add_rows_ms | scratch_ms | branch_MB gather_MB | "
             "gather_over_branch scratch_over_branch | warm_pivots_mean (every parent ended FEASIBLE: no child is cold)"]
    strong = ["# strong branching, 8 candidates per parent, max_pivots = 2: n m0 probes | branch_no_state_ms | "
              "gather_add_rows_ms | branch_MB gather_MB | gather_over_branch | stopped_by_cap"]
    med = statistics.median
    for n, m0 in SHAPES:
        probs = [sx.generateRandomProblem(n, m0, 7919 * k + n * 100 + m0, 1, 100) for k in range(args.parents)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        kept = sx.solve_batch_tensors(A, b, c, keep_state=True)
        assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
        P = args.parents
        x = kept.solution

        # ---- two children per parent
        parent = torch.arange(P, device="cuda").repeat_interleave(2)
        j = x.argmax(dim=1)
        down = torch.floor(x.gather(1, j[:, None]))[:, 0]
        var64 = j.repeat_interleave(2)[:, None]
        sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device="cuda").repeat(P)
        coef = sign[:, None].contiguous()
        rhs = torch.stack([down, -(down + 1.0)], dim=1).reshape(-1, 1).contiguous()
        parent32, var32 = parent.to(torch.int32), var64.to(torch.int32)
        C = parent.shape[0]

        ours = sx.branch_batch_tensors(kept.state, parent32, var32, coef, rhs, A, b, c)
        theirs, (A2, b2) = gather_path(kept.state, parent, var64, coef, rhs, A, b, c)
        c2 = c.index_select(0, parent)
        scratch = sx.solve_batch_tensors(A2, b2, c2)
        assert ours.evicted == 0 and theirs.evicted == 0 and scratch.evicted == 0
        same(ours, theirs)
        assert torch.equal(ours.status, scratch.status)
        fns = [timed(lambda: sx.branch_batch_tensors(kept.state, parent32, var32, coef, rhs, A, b, c)),
               timed(lambda: gather_path(kept.state, parent, var64, coef, rhs, A, b, c)),
               timed(lambda: sx.solve_batch_tensors(A2, b2, c2))]
        seconds_in_turn(fns, args.warmup)
        t_a, t_b, t_c = seconds_in_turn(fns, args.repeats)
        mb_a, mb_b = (v / 1e6 for v in bytes_moved(n, m0, C, True, False))
        line = (f"{n} {m0} {C} | {fmt(t_a)} | {fmt(t_b)} | {fmt(t_c)} | {mb_a:.1f} {mb_b:.1f} | "
                f"{med(t_b) / med(t_a):.2f} {med(t_c) / med(t_a):.2f} | {float(ours.pivots[:, 1].double().mean()):.2f}")
        print(line, flush=True)
        lines.append(line)

        # ---- strong branching: 8 candidates per parent, two dual pivots each, no state kept
        K = 8
        parent = torch.arange(P, device="cuda").repeat_interleave(K)
        cand = x.topk(K, dim=1).indices.reshape(-1, 1)
        rhs = torch.floor(x.gather(1, cand.reshape(P, K))).reshape(-1, 1).contiguous()
        coef = torch.ones_like(rhs)
        parent32, var32 = parent.to(torch.int32), cand.to(torch.int32)
        probe = sx.branch_batch_tensors(kept.state, parent32, var32, coef, rhs, A, b, c, max_pivots=2,
                                        objective_row=True, keep_state=False)
        theirs, _ = gather_path(kept.state, parent, cand, coef, rhs, A, b, c, max_pivots=2, objective_row=True)
        same(probe, theirs, state=False)
        assert torch.equal(probe.objective_row.view(torch.int64), theirs.objective_row.view(torch.int64))
        stopped = int((probe.status == sx.PIVOT_CAP).sum())
        fns = [timed(lambda: sx.branch_batch_tensors(kept.state, parent32, var32, coef, rhs, A, b, c, max_pivots=2,
                                                     objective_row=True, keep_state=False)),
               timed(lambda: gather_path(kept.state, parent, cand, coef, rhs, A, b, c, max_pivots=2, objective_row=True))]
        seconds_in_turn(fns, args.warmup)
        t_a, t_b = seconds_in_turn(fns, args.repeats)
        mb_a = bytes_moved(n, m0, P * K, False, True)[0] / 1e6
        mb_b = bytes_moved(n, m0, P * K, True, True)[1] / 1e6
        line = (f"{n} {m0} {P * K} | {fmt(t_a)} | {fmt(t_b)} | {mb_a:.1f} {mb_b:.1f} | {med(t_b) / med(t_a):.2f} | {stopped}")
        print(line, flush=True)
        strong.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + strong) + "\n")


if __name__ == "__main__":
    main()
