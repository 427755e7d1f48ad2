#!/usr/bin/env python3
"""One large LP held in device tensors: solve_tensors against the host trip it replaces.

For each shape (n x m = 8192 x 4096 and 8192 x 32768, the generated instances of bench.py's config3
and config5, held as contiguous float64 device tensors A [m, n], b [m], c [n]) two paths produce the
solution, the basis and the final objective row as device tensors:

  (a) host trip   Problem.from_arrays(A.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()),
                  twoPhaseMethodEx, last_objective_row, and the three results copied to the device
  (b) tensors     solve_tensors(A, b, c, objective_row=True)

The script first asserts that the two agree in every field, bit for bit (this also warms both up),
then times them with the host clock around work that ends in torch.cuda.synchronize(): the median
and the range of --repeats repeats, the two paths taking turns inside every repeat.  One further
solve of each path, capped at one pivot, runs with the TIMER CSV on and reports its fillTableau step
(the timer changes how the pivots run, so it is kept out of the timed repeats).  The lines are
printed and written to profiles/solve_tensors_bench.txt (or --out).

    python scripts/solve_tensors_bench.py [--repeats 5] [--shapes 8192x4096,8192x32768] [--out FILE]

--trace-only builds each instance and runs one solve_tensors capped at one pivot and nothing else:
the run to put under `rocprofv3 --kernel-trace --stats` for k_build_strided's time, whose achieved
rate is 16 m (1 + n) bytes (the structural block and b read once and written once) over that time.
"""
import argparse
import glob
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import simplexoncuda_amd as sx  # noqa: E402

SEEDS = {(8192, 4096): 823296, (8192, 32768): 851968}  # seed n * 100 + m, as bench.py's configs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_trip(A, b, c, max_pivots=-1):
    """what a caller holding device tensors has to do without solve_tensors"""
    p = sx.Problem.from_arrays(A.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy())
    try:
        r = sx.twoPhaseMethodEx(p, max_pivots)
        row = sx.last_objective_row()
    finally:
        p.close()
    dev = A.device
    out = (r, torch.from_numpy(r.solution).to(dev), torch.from_numpy(r.base).to(dev), torch.from_numpy(row).to(dev))
    torch.cuda.synchronize()
    return out


def tensors(A, b, c, max_pivots=-1):
    out = sx.solve_tensors(A, b, c, max_pivots=max_pivots, objective_row=True)
    torch.cuda.synchronize()
    return out


def assert_same(a, t, n, m):
    r, x, base, row = a
    assert (r.status, tuple(r.pivots), len(row)) == (t.status, tuple(t.pivots), t.row_width)
    assert torch.equal(base, t.base)
    assert np.array_equal(bits(row.cpu().numpy()), bits(t.objective_row[:t.row_width].cpu().numpy()))
    assert not bits(t.objective_row[t.row_width:].cpu().numpy()).any()
    if r.status == sx.FEASIBLE:
        assert bits(r.optimal_value) == bits(t.optimal_value)
        assert np.array_equal(bits(x.cpu().numpy()), bits(t.solution.cpu().numpy()))
    else:
        assert np.isnan(t.optimal_value) and not bits(t.solution.cpu().numpy()).any()


def fill_tableau_us(fn):
    """the fillTableau step (microseconds) of the TIMER CSV of one call of fn"""
    lib = sx.load()
    with tempfile.TemporaryDirectory() as d:
        lib.simplex_set_timer_dir(d.encode())
        try:
            fn()
        finally:
            lib.simplex_set_timer_dir(None)
        (path,) = glob.glob(os.path.join(d, "*.txt"))
        for line in open(path):
            f = line.strip().split(",")
            if len(f) == 4 and f[2] == "fillTableau":
                return float(f[3])
    raise RuntimeError("no fillTableau line in the TIMER CSV")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="8192x4096,8192x32768")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_tensors_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("solve_tensors_bench: no GPU")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    lines = [f"# scripts/solve_tensors_bench.py --repeats {args.repeats} --shapes {args.shapes}",
             "# times in seconds, host clock around work ending in torch.cuda.synchronize(); (a) host trip, (b) solve_tensors",
             "# n m status pivots a_median a_min a_max b_median b_min b_max saved_s a_over_b fill_a_ms fill_b_ms"]
    for n, m in shapes:
        p = sx.generateRandomProblemDevice(n, m, SEEDS.get((n, m), n * 100 + m), 1, 100)
        A, b, c = (torch.from_numpy(a).cuda() for a in p.arrays())
        p.close()
        assert A.shape == (m, n) and A.is_contiguous()
        if args.trace_only:
            t = tensors(A, b, c, max_pivots=1)
            print(f"{n} {m} trace run: status {t.status} pivots {t.pivots}", flush=True)
            continue
        assert_same(host_trip(A, b, c), tensors(A, b, c), n, m)
        ta, tb = [], []
        for _ in range(args.repeats):
            for ts, fn in ((ta, host_trip), (tb, tensors)):
                t0 = time.perf_counter()
                out = fn(A, b, c)
                ts.append(time.perf_counter() - t0)
        r = out if isinstance(out, sx.SolveTensors) else out[0]
        fa = fill_tableau_us(lambda: host_trip(A, b, c, max_pivots=1))
        fb = fill_tableau_us(lambda: tensors(A, b, c, max_pivots=1))
        ma, mb = statistics.median(ta), statistics.median(tb)
        line = (f"{n} {m} {r.status} {r.pivots[0]}+{r.pivots[1]} {ma:.3f} {min(ta):.3f} {max(ta):.3f} "
                f"{mb:.3f} {min(tb):.3f} {max(tb):.3f} {ma - mb:.3f} {ma / mb:.2f} {fa / 1e3:.1f} {fb / 1e3:.1f}")
        print(line, flush=True)
        lines.append(line)
        del A, b, c
        torch.cuda.empty_cache()
    if args.trace_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
