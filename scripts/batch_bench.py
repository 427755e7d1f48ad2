#!/usr/bin/env python3
"""Batched solve against a loop of single solves, in LPs per second.

For each shape (32x16 and 64x64: n variables x m constraints, values in [1,100]) 1024 generated
instances are solved with one solve_batch call (wall time around the call, after warm-up; the
median of several repeats), and a 64-problem subset of the same instances with a loop of
twoPhaseMethodEx, the one-problem entry point.  The same instances, stacked once into device
tensors, are also solved with solve_batch_tensors (default arguments, and objective_row=True): the
same host clock, each call followed by torch.cuda.synchronize(), the three batched paths taking
turns inside every repeat.  The rates are printed and written to profiles/batch_bench.txt (or --out).

    python scripts/batch_bench.py [--problems 1024] [--subset 64] [--repeats 7] [--out FILE]
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


def median_seconds(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def median_seconds_in_turn(fns, repeats):
    """the medians of several functions timed one after the other inside every repeat"""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for ts, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return [statistics.median(ts) for ts in times]


def device_tensors(probs):
    """A [B, m, n], b [B, m], c [B, n] of the problems, on the GPU"""
    arrays = [p.arrays() for p in probs]
    return tuple(torch.from_numpy(np.stack([a[k] for a in arrays])).cuda() for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.txt"))
    args = ap.parse_args()

    lines = [f"# scripts/batch_bench.py --problems {args.problems} --subset {args.subset} --repeats {args.repeats}",
             "# n m problems class batch_LPs_per_s loop_LPs_per_s ratio batch_ms loop_ms_per_LP "
             "tensors_ms tensors_row_ms batch_ms_over_tensors_ms"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
        subset = probs[:args.subset]
        # the two paths agree on the subset (and this warms both up)
        got = sx.solve_batch(probs)
        for p, g in zip(subset, got):
            one = sx.twoPhaseMethodEx(p)
            assert (one.status, tuple(one.pivots), one.optimal_value) == (g.status, tuple(g.pivots), g.optimal_value)
        # the tensor path gives solve_batch's status, pivots and objective on every instance
        A, b, c = device_tensors(probs)
        ten = sx.solve_batch_tensors(A, b, c)
        status, pivots, opt = ten.status.cpu().numpy(), ten.pivots.cpu().numpy(), ten.optimal_value.cpu().numpy()
        for k, g in enumerate(got):
            assert (g.status, tuple(g.pivots)) == (int(status[k]), tuple(int(v) for v in pivots[k])), k
            assert g.status != sx.FEASIBLE or g.optimal_value == opt[k], k
        sx.solve_batch_tensors(A, b, c, objective_row=True)

        def tensors(row):
            sx.solve_batch_tensors(A, b, c, objective_row=row)
            torch.cuda.synchronize()

        sx.solve_batch(probs)
        t_batch, t_ten, t_row = median_seconds_in_turn(
            [lambda: sx.solve_batch(probs), lambda: tensors(False), lambda: tensors(True)], args.repeats)
        t_loop = median_seconds(lambda: [sx.twoPhaseMethodEx(p) for p in subset], max(3, args.repeats // 2))
        r_batch, r_loop = len(probs) / t_batch, len(subset) / t_loop
        line = (f"{n} {m} {len(probs)} {sx.batch_class(n, m)} {r_batch:.0f} {r_loop:.0f} {r_batch / r_loop:.1f} "
                f"{t_batch * 1e3:.3f} {t_loop / len(subset) * 1e3:.3f} "
                f"{t_ten * 1e3:.3f} {t_row * 1e3:.3f} {t_batch / t_ten:.1f}")
        print(line, flush=True)
        lines.append(line)
        for p in probs:
            p.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
