#!/usr/bin/env python3
"""One Gomory mixed-integer cut per problem from a kept batch state, on the device, against what a caller
had to do without the entry.

For each shape (32x16 and 64x64: n variables x m constraints, values in [1,100], b times --scale so that
the optima are not all below 1) 1024 generated problems are solved once with keep_state=True; every
variable is integer.  Three paths to the problems with one cut each take turns inside every repeat, each
call followed by torch.cuda.synchronize() under one host clock:

  (a) cut       sx.cut_batch_tensors into a preallocated envelope A [B, m + 1, n], b [B, m + 1];
  (b) torch     what a caller does without it: the same formula written in torch on the device from
                state.T, state.base, A and b (the layout of the kept tableau is DESIGN.md §10.4's), the
                row appended with torch.cat, then sx.add_rows_batch_tensors -- all of it inside the timed
                call, since all of it is repeated in every round;
  (c) scratch   sx.solve_batch_tensors on (b)'s grown problems (made once, outside the clock).

(a) and (b) are asserted to choose the same source rows, to agree in cut_A and cut_b to rounding and to end
in the same statuses, and (c) to end in them too.  Printed per path: the median, the minimum and the
maximum of the repeats, and the share of problems that yield a cut.  Written to profiles/cut_bench.txt (or
--out).

    python scripts/cut_bench.py [--problems 1024] [--scale 37] [--repeats 21] [--warmup 3] [--out FILE]
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
AWAY = 0.05
EPS = 1e-9


def seconds_in_turn(fns, repeats):
    """every time of several functions timed one after the other inside every repeat"""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for ts, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return times


def device_tensors(probs, scale):
    """A [B, m, n], b [B, m] times scale, c [B, n] of the problems, on the GPU"""
    arrays = [p.arrays() for p in probs]
    A, b, c = (torch.from_numpy(np.stack([a[k] for a in arrays])).cuda() for k in range(3))
    return A, b * float(scale), c


def torch_cut(state, A0, b0, mask):
    """(cut_A [B, n], cut_b [B], row [B], -1 for none) of one GMI cut per problem, every kept problem taken
    for an optimum: the formula of simplex_solve_batch_device_cut in batched torch operations (plain
    multiply-add, torch's argmin in place of the solver's eps-argmin tree)"""
    B, m0, n = A0.shape
    T, v = state.T, state.base.long()
    ar = torch.arange(B, device=T.device)
    t0 = T[:, :, 0]
    f0 = t0 - torch.floor(t0)
    near = torch.minimum(f0, 1.0 - f0)
    elig = (v < n) & mask[v.clamp(max=n - 1)] & (f0 >= AWAY) & (1.0 - f0 >= AWAY)
    key = torch.where(elig, -near, torch.full_like(near, float("inf")))
    r = key.argmin(dim=1)
    has = elig.any(dim=1)
    alpha = T[ar, r, 1:1 + n + m0]
    f0r = f0[ar, r][:, None]
    rho = f0r / (1.0 - f0r)
    basic = torch.zeros((B, n + m0), dtype=torch.bool, device=T.device).scatter_(1, v, True)
    fj = alpha - torch.floor(alpha)
    g_int = torch.where(fj <= f0r, fj, rho * (1.0 - fj))
    g_cont = torch.where(alpha > 0, alpha, rho * (-alpha))
    intcol = torch.cat([mask.expand(B, n), torch.zeros((B, m0), dtype=torch.bool, device=T.device)], dim=1)
    g = torch.where(intcol, g_int, g_cont)
    g = torch.where(basic | (alpha.abs() < EPS) | ~has[:, None], torch.zeros_like(g), g)
    cut_A = torch.bmm(g[:, None, n:], A0)[:, 0] - g[:, :n]
    cut_b = (g[:, n:] * b0).sum(dim=1) - torch.where(has, f0r[:, 0], torch.zeros_like(f0r[:, 0]))
    return cut_A, cut_b, torch.where(has, r, torch.full_like(r, -1))


def torch_path(state, A0, b0, c, mask):
    """a caller without the cut entry: the cut in torch, the grown problem by torch.cat, add_rows"""
    cut_A, cut_b, row = torch_cut(state, A0, b0, mask)
    A2 = torch.cat([A0, cut_A[:, None]], dim=1)
    b2 = torch.cat([b0, cut_b[:, None]], dim=1)
    return sx.add_rows_batch_tensors(state, A2, b2, c), (A2, b2, row)


def timed(fn):
    def run():
        fn()
        torch.cuda.synchronize()
    return run


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:.3f} ({min(ts) * 1e3:.3f} - {max(ts) * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=37.0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cut_bench.py measures on a GPU; none is available")
    torch.cuda.set_device(0)
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.problems} problems, b times {args.scale:g}, every variable integer, "
             f"one cut per problem, away = {AWAY}; {args.warmup} warm-up and {args.repeats} timed repeats per path, in "
             "turn; times in ms as median (min - max)",
             "# n m0 | share_with_a_cut | cut_ms | torch_add_rows_ms | scratch_ms | torch_over_cut scratch_over_cut | "
             "largest relative difference of the emitted rows (a) against (b) | dual_pivots_mean"]
    med = statistics.median
    for n, m0 in SHAPES:
        probs = [sx.generateRandomProblem(n, m0, 7919 * k + n * 100 + m0, 1, 100) for k in range(args.problems)]
        A0, b0, c = device_tensors(probs, args.scale)
        for p in probs:
            p.close()
        B = args.problems
        kept = sx.solve_batch_tensors(A0, b0, c, keep_state=True)
        assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
        mask = torch.ones(n, dtype=torch.bool, device="cuda")
        A = torch.zeros((B, m0 + 1, n), dtype=torch.float64, device="cuda")  # the envelope, allocated once
        b = torch.zeros((B, m0 + 1), dtype=torch.float64, device="cuda")
        A[:, :m0] = A0
        b[:, :m0] = b0

        ours = sx.cut_batch_tensors(kept.state, A, b, c, mask, away=AWAY)
        theirs, (A2, b2, row) = torch_path(kept.state, A0, b0, c, mask)
        scratch = sx.solve_batch_tensors(A2, b2, c)
        assert ours.evicted == 0 and theirs.evicted == 0 and scratch.evicted == 0
        assert torch.equal(ours.cut_rows[:, 0].long(), row), "the two paths chose different source rows"
        share = float((row >= 0).double().mean())
        assert share >= 0.9, f"only {share:.3f} of the problems yield a cut; raise --scale"
        scale_A = A2[:, m0].abs().amax(dim=1).clamp(min=1.0)
        diff = max(float(((A[:, m0] - A2[:, m0]).abs().amax(dim=1) / scale_A).max()),
                   float(((b[:, m0] - b2[:, m0]).abs() / b2[:, m0].abs().clamp(min=1.0)).max()))
        assert diff <= 1e-9, diff  # rounding: another order of the same sum of m0 products
        assert torch.equal(ours.status, theirs.status) and torch.equal(ours.status, scratch.status)
        fns = [timed(lambda: sx.cut_batch_tensors(kept.state, A, b, c, mask, away=AWAY)),
               timed(lambda: torch_path(kept.state, A0, b0, c, mask)),
               timed(lambda: sx.solve_batch_tensors(A2, b2, c))]
        seconds_in_turn(fns, args.warmup)
        t_a, t_b, t_c = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m0} | {share:.3f} | {fmt(t_a)} | {fmt(t_b)} | {fmt(t_c)} | "
                f"{med(t_b) / med(t_a):.2f} {med(t_c) / med(t_a):.2f} | {diff:.1e} | "
                f"{float(ours.pivots[:, 1].double().mean()):.2f}")
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
