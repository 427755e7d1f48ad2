#!/usr/bin/env python3
"""Batched solve against a loop of single solves, in LPs per second.

For each shape (32x16 and 64x64: n variables x m constraints, values in [1,100]) 1024 generated
instances are solved with one solve_batch call (wall time around the call, after warm-up; the
median of several repeats), and a 64-problem subset of the same instances with a loop of
twoPhaseMethodEx, the one-problem entry point.  The same instances, stacked once into device
tensors, are also solved with solve_batch_tensors (default arguments, and objective_row=True): the
same host clock, each call followed by torch.cuda.synchronize(), the three batched paths taking
turns inside every repeat.  The ragged leg (ragged_leg below) then times the ragged device entry
against the one-shape entry on the same uniform instances, and against solve_batch on problems whose
dimensions vary inside a 64 x 64 envelope; the state leg (state_leg) what keeping the batch state
costs and what a warm start from it saves; the rhs leg (rhs_leg) what re-solving the kept state for a
new right-hand side saves; the rows leg (rows_leg) what adding a cut to the kept state saves; the cols
leg (cols_leg) what adding a priced-in column to it saves; the drop leg (drop_leg) what taking that cut or that
column out of the kept state again saves.  The rates are printed and written to profiles/batch_bench.txt (or --out).

    python scripts/batch_bench.py [--problems 1024] [--subset 64] [--repeats 7]
                                  [--legs all|uniform|ragged|state|rhs|rows|cols|drop] [--out FILE]
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


def seconds_in_turn(fns, repeats):
    """every time of several functions timed one after the other inside every repeat"""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for ts, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return times


def ragged_leg(args):
    """The ragged device entry (solve_batch_tensors(n_active=, m_active=)), two questions.

    Cost of raggedness: the SHAPES' instances with every block fully active, the ragged entry (default
    order, and order=False) and the one-shape entry taking turns inside every repeat; the yardstick
    is the one-shape entry of the same run, whose own spread (min and max of its repeats) is printed.

    The use case: as many LPs with n_k and m_k drawn uniformly from 8..64, in a (64, 64) envelope,
    through the ragged entry (default order, order=False) and through the host path solve_batch on
    the same problems, after asserting that status, pivots and objective agree on every instance;
    and a batch of small problems whose few large ones come last, the case the order exists for."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    lines = ["# ragged, uniform dims: n m problems one_shape_ms one_shape_min_ms one_shape_max_ms ragged_ms "
             "ragged_order_false_ms ragged_over_one_shape"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        n_k = torch.full((len(probs),), n, dtype=torch.int32, device="cuda")
        m_k = torch.full((len(probs),), m, dtype=torch.int32, device="cuda")
        one = sx.solve_batch_tensors(A, b, c, objective_row=True)
        rag = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k)
        for f in ("status", "pivots", "base", "row_width"):
            assert torch.equal(getattr(one, f), getattr(rag, f)), f
        for f in ("optimal_value", "solution", "objective_row"):
            assert torch.equal(getattr(one, f).view(torch.int64), getattr(rag, f).view(torch.int64)), f

        def call(**kw):
            sx.solve_batch_tensors(A, b, c, **kw)
            torch.cuda.synchronize()

        fns = [lambda: call(), lambda: call(n_active=n_k, m_active=m_k),
               lambda: call(n_active=n_k, m_active=m_k, order=False)]
        seconds_in_turn(fns, 2)  # warm-up
        t_one, t_rag, t_raw = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m} {len(probs)} {ms(t_one)} {min(t_one) * 1e3:.3f} {max(t_one) * 1e3:.3f} {ms(t_rag)} {ms(t_raw)} "
                f"{statistics.median(t_rag) / statistics.median(t_one):.3f}")
        print(line, flush=True)
        lines.append(line)

    lines.append("# ragged, dims inside a 64 x 64 envelope (uniform: n_k, m_k uniform in 8..64; tail: 8..16 but for the last "
                 "sixteenth of the batch, 56..64): draw problems solve_batch_ms ragged_ms solve_batch_ms_over_ragged_ms | "
                 "in turn: ragged_default_order_ms ragged_order_false_ms ragged_order_given_ms")
    rng = np.random.default_rng(64)
    uniform = rng.integers(8, 65, size=(args.problems, 2))
    tail = np.concatenate([rng.integers(8, 17, size=(args.problems - args.problems // 16, 2)),
                           rng.integers(56, 65, size=(args.problems // 16, 2))])
    for draw, dims in (("uniform", uniform), ("tail", tail)):
        line = f"{draw} " + mixed_dims_case(args, dims, 64, 64)
        print(line, flush=True)
        lines.append(line)
    return lines


def state_leg(args):
    """The batch state (solve_batch_tensors(keep_state=True), resume_batch_tensors), two questions on
    the SHAPES' instances, the four calls taking turns inside every repeat: what keeping the state
    costs (the same solve with and without it), and what the warm start saves -- new costs
    c (1 + 0.1 u), u uniform in [-1, 1], solved by re-costing the kept optimum (recost=True, into a
    new state, so every repeat starts from the same one) and from scratch, after asserting that both
    end in the same status on every instance."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    med = statistics.median
    lines = ["# state: n m problems solve_ms solve_min_ms solve_max_ms keep_state_ms keep_over_solve recost_ms "
             "scratch_new_costs_ms scratch_over_recost warm_pivots_mean scratch_pivots_mean"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        u = torch.from_numpy(np.random.default_rng(n * 100 + m).uniform(-1.0, 1.0, size=tuple(c.shape))).cuda()
        c2 = c * (1.0 + 0.1 * u)
        kept = sx.solve_batch_tensors(A, b, c, keep_state=True)
        warm = sx.resume_batch_tensors(kept.state, c2, recost=True, in_place=False)
        scratch = sx.solve_batch_tensors(A, b, c2)
        assert kept.evicted == 0 and warm.evicted == 0 and scratch.evicted == 0
        assert torch.equal(warm.status, scratch.status)
        piv_warm = float(warm.pivots[:, 1].double().mean())
        piv_scratch = float(scratch.pivots.sum(dim=1).double().mean())

        def timed(fn):
            def run():
                fn()
                torch.cuda.synchronize()
            return run

        fns = [timed(lambda: sx.solve_batch_tensors(A, b, c)),
               timed(lambda: sx.solve_batch_tensors(A, b, c, keep_state=True)),
               timed(lambda: sx.resume_batch_tensors(kept.state, c2, recost=True, in_place=False)),
               timed(lambda: sx.solve_batch_tensors(A, b, c2))]
        seconds_in_turn(fns, 2)  # warm-up
        t_one, t_keep, t_warm, t_new = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m} {len(probs)} {ms(t_one)} {min(t_one) * 1e3:.3f} {max(t_one) * 1e3:.3f} {ms(t_keep)} "
                f"{med(t_keep) / med(t_one):.3f} {ms(t_warm)} {ms(t_new)} {med(t_new) / med(t_warm):.2f} "
                f"{piv_warm:.1f} {piv_scratch:.1f}")
        print(line, flush=True)
        lines.append(line)
    return lines


def rhs_leg(args):
    """A new right-hand side on the kept state (resume_batch_tensors(state, c, A=, b=)) on the SHAPES'
    instances: b (1 + 0.1 u), u uniform in [-1, 1], solved warm from the kept optimum (the dual
    simplex, into a new state, so every repeat starts from the same one) and from scratch, the two
    calls taking turns inside every repeat, after asserting that both end in the same status on every
    instance."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    med = statistics.median
    lines = ["# rhs: n m problems rerhs_ms rerhs_min_ms rerhs_max_ms scratch_new_b_ms scratch_min_ms scratch_max_ms "
             "scratch_over_rerhs warm_pivots_mean scratch_pivots_mean"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        u = torch.from_numpy(np.random.default_rng(n * 100 + m).uniform(-1.0, 1.0, size=tuple(b.shape))).cuda()
        b2 = b * (1.0 + 0.1 * u)
        kept = sx.solve_batch_tensors(A, b, c, keep_state=True)
        warm = sx.resume_batch_tensors(kept.state, c, A=A, b=b2, in_place=False)
        scratch = sx.solve_batch_tensors(A, b2, c)
        assert kept.evicted == 0 and warm.evicted == 0 and scratch.evicted == 0
        assert torch.equal(warm.status, scratch.status)
        piv_warm = float(warm.pivots[:, 1].double().mean())
        piv_scratch = float(scratch.pivots.sum(dim=1).double().mean())

        def timed(fn):
            def run():
                fn()
                torch.cuda.synchronize()
            return run

        fns = [timed(lambda: sx.resume_batch_tensors(kept.state, c, A=A, b=b2, in_place=False)),
               timed(lambda: sx.solve_batch_tensors(A, b2, c))]
        seconds_in_turn(fns, 2)  # warm-up
        t_warm, t_new = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m} {len(probs)} {ms(t_warm)} {min(t_warm) * 1e3:.3f} {max(t_warm) * 1e3:.3f} {ms(t_new)} "
                f"{min(t_new) * 1e3:.3f} {max(t_new) * 1e3:.3f} {med(t_new) / med(t_warm):.2f} "
                f"{piv_warm:.1f} {piv_scratch:.1f}")
        print(line, flush=True)
        lines.append(line)
    return lines


def rows_leg(args):
    """A new constraint row on the kept state (add_rows_batch_tensors) on the SHAPES' instances: every
    kept optimum x* gets one cut a x <= beta with a = A[0], a positive row, and beta = 0.5 a x*, solved
    warm from the kept optimum (the dual simplex on the grown state) and from scratch on the grown
    problem, the two calls taking turns inside every repeat, after asserting that both end in the
    same status on every instance."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    med = statistics.median
    lines = ["# rows: n m0 problems add_row_ms add_row_min_ms add_row_max_ms scratch_grown_ms scratch_min_ms scratch_max_ms "
             "scratch_over_add_row warm_pivots_mean scratch_pivots_mean"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        kept = sx.solve_batch_tensors(A, b, c, keep_state=True)
        assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
        a = A[:, 0, :]
        beta = 0.5 * (a * kept.solution).sum(dim=1)
        A2 = torch.cat([A, a[:, None, :]], dim=1).contiguous()
        b2 = torch.cat([b, beta[:, None]], dim=1).contiguous()
        warm = sx.add_rows_batch_tensors(kept.state, A2, b2, c)
        scratch = sx.solve_batch_tensors(A2, b2, c)
        assert warm.evicted == 0 and scratch.evicted == 0
        assert torch.equal(warm.status, scratch.status)
        piv_warm = float(warm.pivots[:, 1].double().mean())
        piv_scratch = float(scratch.pivots.sum(dim=1).double().mean())

        def timed(fn):
            def run():
                fn()
                torch.cuda.synchronize()
            return run

        fns = [timed(lambda: sx.add_rows_batch_tensors(kept.state, A2, b2, c)),
               timed(lambda: sx.solve_batch_tensors(A2, b2, c))]
        seconds_in_turn(fns, 2)  # warm-up
        t_warm, t_new = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m} {len(probs)} {ms(t_warm)} {min(t_warm) * 1e3:.3f} {max(t_warm) * 1e3:.3f} {ms(t_new)} "
                f"{min(t_new) * 1e3:.3f} {max(t_new) * 1e3:.3f} {med(t_new) / med(t_warm):.2f} "
                f"{piv_warm:.1f} {piv_scratch:.1f}")
        print(line, flush=True)
        lines.append(line)
    return lines


def cols_leg(args):
    """A new variable on the kept state (add_cols_batch_tensors): instances of n + 1 variables for the
    SHAPES' (n, m), the state kept of their first n columns; the last column a gets the cost
    1.5 y a + 1, y the kept duals (the slack entries of the kept objective row), so it prices in on
    every instance.  Solved warm from the kept optimum (phase 2 on the grown state) and from scratch
    on the grown problem, the two calls taking turns inside every repeat, after asserting that both
    end in the same status on every instance."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    med = statistics.median
    lines = ["# cols: n0 m problems add_col_ms add_col_min_ms add_col_max_ms scratch_grown_ms scratch_min_ms scratch_max_ms "
             "scratch_over_add_col warm_pivots_mean scratch_pivots_mean"]
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n + 1, m, 7919 * k + (n + 1) * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        kept = sx.solve_batch_tensors(A[:, :, :n], b, c[:, :n], keep_state=True)
        assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
        y = kept.state.d[:, 1 + n:1 + n + m]
        c2 = c.clone()
        c2[:, n] = 1.5 * (y * A[:, :, n]).sum(dim=1) + 1.0
        warm = sx.add_cols_batch_tensors(kept.state, A, b, c2)
        scratch = sx.solve_batch_tensors(A, b, c2)
        assert warm.evicted == 0 and scratch.evicted == 0
        assert torch.equal(warm.status, scratch.status)
        assert bool((warm.pivots[:, 1] >= 1).all())
        piv_warm = float(warm.pivots[:, 1].double().mean())
        piv_scratch = float(scratch.pivots.sum(dim=1).double().mean())

        def timed(fn):
            def run():
                fn()
                torch.cuda.synchronize()
            return run

        fns = [timed(lambda: sx.add_cols_batch_tensors(kept.state, A, b, c2)),
               timed(lambda: sx.solve_batch_tensors(A, b, c2))]
        seconds_in_turn(fns, 2)  # warm-up
        t_warm, t_new = seconds_in_turn(fns, args.repeats)
        line = (f"{n} {m} {len(probs)} {ms(t_warm)} {min(t_warm) * 1e3:.3f} {max(t_warm) * 1e3:.3f} {ms(t_new)} "
                f"{min(t_new) * 1e3:.3f} {max(t_new) * 1e3:.3f} {med(t_new) / med(t_warm):.2f} "
                f"{piv_warm:.1f} {piv_scratch:.1f}")
        print(line, flush=True)
        lines.append(line)
    return lines


def drop_leg(args):
    """A row or a column taken out of the kept state again (drop_rows_batch_tensors,
    drop_cols_batch_tensors), three cases on the SHAPES' instances: the rows leg's cut a x <= theta a x*
    added by add_rows_batch_tensors at theta = 0.5 (binding: its slack is forced into the basis first)
    and at theta = 1.5 (its slack is basic: no pivot) and dropped from the grown state; the cols leg's
    priced-in column added by add_cols_batch_tensors and dropped again.  Each against solve_batch_tensors
    on the reduced problem, the two calls taking turns inside every repeat, after asserting that both end
    in the same status on every instance."""
    ms = lambda t: f"{statistics.median(t) * 1e3:.3f}"  # noqa: E731
    med = statistics.median
    lines = ["# drop: case n_in m_in problems drop_ms drop_min_ms drop_max_ms scratch_reduced_ms scratch_min_ms "
             "scratch_max_ms scratch_over_drop warm_pivots_mean scratch_pivots_mean   (warm pivots: forced ones included)"]

    def timed(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run

    def measure(case, grown, fn, small):
        warm = fn()
        scratch = sx.solve_batch_tensors(*small)
        assert warm.evicted == 0 and scratch.evicted == 0
        assert torch.equal(warm.status, scratch.status)
        piv_warm = float(warm.pivots[:, 1].double().mean())
        piv_scratch = float(scratch.pivots.sum(dim=1).double().mean())
        fns = [timed(fn), timed(lambda: sx.solve_batch_tensors(*small))]
        seconds_in_turn(fns, 2)  # warm-up
        t_warm, t_new = seconds_in_turn(fns, args.repeats)
        line = (f"{case} {grown.n} {grown.m} {small[0].shape[0]} {ms(t_warm)} {min(t_warm) * 1e3:.3f} "
                f"{max(t_warm) * 1e3:.3f} {ms(t_new)} {min(t_new) * 1e3:.3f} {max(t_new) * 1e3:.3f} "
                f"{med(t_new) / med(t_warm):.2f} {piv_warm:.1f} {piv_scratch:.1f}")
        print(line, flush=True)
        lines.append(line)

    for theta in (0.5, 1.5):
        for n, m in SHAPES:
            probs = [sx.generateRandomProblem(n, m, 7919 * k + n * 100 + m, 1, 100) for k in range(args.problems)]
            A, b, c = device_tensors(probs)
            for p in probs:
                p.close()
            kept = sx.solve_batch_tensors(A, b, c, keep_state=True)
            assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
            a = A[:, 0, :]
            beta = theta * (a * kept.solution).sum(dim=1)
            A2 = torch.cat([A, a[:, None, :]], dim=1).contiguous()
            b2 = torch.cat([b, beta[:, None]], dim=1).contiguous()
            grown = sx.add_rows_batch_tensors(kept.state, A2, b2, c)
            assert grown.evicted == 0
            rows = torch.full((len(probs), 1), m, dtype=torch.int32, device="cuda")
            measure(f"row_theta_{theta}", grown.state, lambda: sx.drop_rows_batch_tensors(grown.state, rows, A, b, c),
                    (A, b, c))
    for n, m in SHAPES:
        probs = [sx.generateRandomProblem(n + 1, m, 7919 * k + (n + 1) * 100 + m, 1, 100) for k in range(args.problems)]
        A, b, c = device_tensors(probs)
        for p in probs:
            p.close()
        A0, c0 = A[:, :, :n].contiguous(), c[:, :n].contiguous()
        kept = sx.solve_batch_tensors(A0, b, c0, keep_state=True)
        assert kept.evicted == 0 and bool((kept.status == sx.FEASIBLE).all())
        y = kept.state.d[:, 1 + n:1 + n + m]
        c2 = c.clone()
        c2[:, n] = 1.5 * (y * A[:, :, n]).sum(dim=1) + 1.0
        grown = sx.add_cols_batch_tensors(kept.state, A, b, c2)
        assert grown.evicted == 0 and bool((grown.pivots[:, 1] >= 1).all())
        cols = torch.full((len(probs), 1), n, dtype=torch.int32, device="cuda")
        measure("priced_in_col", grown.state, lambda: sx.drop_cols_batch_tensors(grown.state, cols, A0, b, c0),
                (A0, b, c0))
    return lines


def mixed_dims_case(args, dims, n, m):
    """problems of the given (n_k, m_k) in an n x m envelope whose padding is NaN: solve_batch on the
    host problems and the ragged entry in turn; then the ragged entry with its default order (built
    inside the call), with order=False and with the same larger-first order passed in, in turn"""
    probs = [sx.generateRandomProblem(int(nk), int(mk), 7919 * k + int(nk) * 100 + int(mk), 1, 100)
             for k, (nk, mk) in enumerate(dims)]
    Ae, be, ce = (np.full(s, np.nan) for s in ((len(probs), m, n), (len(probs), m), (len(probs), n)))
    for k, p in enumerate(probs):
        Ak, bk, ck = p.arrays()
        Ae[k, :p.m, :p.n], be[k, :p.m], ce[k, :p.n] = Ak, bk, ck
    A, b, c = (torch.from_numpy(t).cuda() for t in (Ae, be, ce))
    n_k = torch.from_numpy(dims[:, 0].astype(np.int32)).cuda()
    m_k = torch.from_numpy(dims[:, 1].astype(np.int32)).cuda()
    got = sx.solve_batch(probs)
    rag = sx.solve_batch_tensors(A, b, c, n_active=n_k, m_active=m_k)
    assert rag.evicted == 0
    status, pivots, opt = rag.status.cpu().numpy(), rag.pivots.cpu().numpy(), rag.optimal_value.cpu().numpy()
    for k, g in enumerate(got):
        assert (g.status, tuple(g.pivots)) == (int(status[k]), tuple(int(v) for v in pivots[k])), k
        assert g.status != sx.FEASIBLE or g.optimal_value == opt[k], k

    def call(**kw):
        sx.solve_batch_tensors(A, b, c, n_active=n_k, m_active=m_k, **kw)
        torch.cuda.synchronize()

    # the host path against the ragged call that follows it, then the three orders among themselves (a call
    # right behind the host-heavy solve_batch is slower than the same call behind a tensor call)
    fns = [lambda: sx.solve_batch(probs), lambda: call()]
    seconds_in_turn(fns, 2)  # warm-up
    t_host, t_rag = (statistics.median(t) for t in seconds_in_turn(fns, args.repeats))
    given = sx.api._default_ragged_order(n_k, m_k)
    fns = [lambda: call(), lambda: call(order=False), lambda: call(order=given)]
    seconds_in_turn(fns, 2)  # warm-up
    t_def, t_raw, t_giv = (statistics.median(t) for t in seconds_in_turn(fns, args.repeats))
    for p in probs:
        p.close()
    return (f"{len(probs)} {t_host * 1e3:.3f} {t_rag * 1e3:.3f} {t_host / t_rag:.1f} "
            f"{t_def * 1e3:.3f} {t_raw * 1e3:.3f} {t_giv * 1e3:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legs", choices=["all", "uniform", "ragged", "state", "rhs", "rows", "cols", "drop"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.txt"))
    args = ap.parse_args()

    lines = [f"# scripts/batch_bench.py --problems {args.problems} --subset {args.subset} --repeats {args.repeats}"
             + ("" if args.legs == "all" else f" --legs {args.legs}")]
    if args.legs in ("all", "uniform"):
        lines.append("# n m problems class batch_LPs_per_s loop_LPs_per_s ratio batch_ms loop_ms_per_LP "
                     "tensors_ms tensors_row_ms batch_ms_over_tensors_ms")
    for n, m in SHAPES if args.legs in ("all", "uniform") else []:
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
    if args.legs in ("all", "ragged"):
        lines += ragged_leg(args)
    if args.legs in ("all", "state"):
        lines += state_leg(args)
    if args.legs in ("all", "rhs"):
        lines += rhs_leg(args)
    if args.legs in ("all", "rows"):
        lines += rows_leg(args)
    if args.legs in ("all", "cols"):
        lines += cols_leg(args)
    if args.legs in ("all", "drop"):
        lines += drop_leg(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
