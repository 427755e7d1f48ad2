"""The batch state (simplex_solve_batch_device_state) restated from the oracle's pieces --
build_phase1, update_objective and solve on a caller's T, d, base -- and nothing else, for
test_batch_state_host.py (the oracle alone) and test_gpu_batch_state.py (bit for bit against the GPU).

A reference state is a dict:

  T        [m, 1 + n + m]   the stored columns b | structural | slack
  d        [1 + n + 2m]     the objective row; +0.0 on [1 + n + m, 1 + n + 2m) in phase 2
  base     int32 [m]
  phase    1 or 2
  pivots   (phase 1, phase 2)
  status, x, opt, row       what the entry reports: oracle.two_phase's fields and the final objective
                            row (x zero and opt NaN unless FEASIBLE, as the device entries write them)
  art      [m, m]           the artificial block of a phase-1 state (None in phase 2): kept only so
                            that a test can show it equals the slack block; a resume does not read it
"""
import numpy as np
import torch

import oracle
import simplexoncuda_amd as sx

EPS = 1e-9
_REF = {}


def _negative(x):
    """compare(x, 0) < 0 (macro.h)"""
    return not abs(x) < EPS and x < 0


def _left(max_pivots, done):
    """the cap orc_solve gets when `done` pivots of the phase's total are behind it"""
    return -1 if max_pivots < 0 else max(max_pivots - done, 0)


def _run(T, d, base, phase, pivots, c, max_pivots, recost):
    """the loop of orc_two_phase entered at a state: T [m, 1 + n + 2m] (phase 1) or [m, 1 + n + m]
    (phase 2), d at full width; all three are written"""
    m = T.shape[0]
    n = len(d) - 1 - 2 * m
    Ns, N1 = 1 + n + m, 1 + n + 2 * m
    p1, p2 = pivots
    art = None
    if phase == 1:
        st, k = oracle.solve(T, d, base, _left(max_pivots, p1))
        p1 += k
        if st == oracle.PIVOT_CAP:
            status = oracle.PIVOT_CAP
        elif _negative(d[0]):
            status = oracle.INFEASIBLE
        elif ((base >= n + m) & (base < n + 2 * m)).any():
            status = oracle.DEGENERATE
        else:
            status = oracle.FEASIBLE
        if status == oracle.FEASIBLE:
            phase, p2, recost = 2, 0, False
            T = np.ascontiguousarray(T[:, :Ns])
            d[1:1 + n] = -c
            d[1 + n:Ns] = 0.0
            d2 = d[:Ns].copy()
            oracle.update_objective(T, d2, base)
            d[:Ns] = d2
        else:
            art = T[:, Ns:].copy()
    if phase == 2:
        d2 = d[:Ns].copy()
        if recost:
            d2[0] = 0.0
            d2[1:1 + n] = -c
            d2[1 + n:] = 0.0
            oracle.update_objective(T, d2, base)
            p2 = 0
        status, k = oracle.solve(T, d2, base, _left(max_pivots, p2))
        p2 += k
        d[:Ns] = d2
        d[Ns:] = 0.0
    feasible = status == oracle.FEASIBLE
    x = np.zeros(n)
    if feasible:
        for i in range(m):
            if base[i] < n:
                x[base[i]] = T[i, 0]
    return {"T": np.ascontiguousarray(T[:, :Ns]), "d": d, "base": base, "phase": phase, "pivots": (int(p1), int(p2)),
            "status": status, "x": x, "opt": d[0] if feasible else float("nan"),
            "row": d[:Ns].copy() if phase == 2 else d.copy(), "art": art}


def ref_state(A, b, c, max_pivots=-1):
    """the state and results of a fresh solve; computed once per instance and cap: do not write it"""
    key = (A.tobytes(), b.tobytes(), c.tobytes(), A.shape, max_pivots)
    if key not in _REF:
        T, d, base = oracle.build_phase1(A, b)
        oracle.update_objective(T, d, base)
        _REF[key] = _run(T, d, base, 1, (0, 0), c, max_pivots, False)
    return _REF[key]


def ref_resume(state, c, max_pivots=-1, recost=False):
    """the state and results of a resume of `state` (which is left as it is)"""
    T, d, base = state["T"].copy(), state["d"].copy(), state["base"].copy()
    if state["phase"] == 1:  # the artificial block is the slack block
        n = T.shape[1] - 1 - T.shape[0]
        T = np.ascontiguousarray(np.concatenate([T, T[:, 1 + n:]], axis=1))
    return _run(T, d, base, state["phase"], state["pivots"], c, max_pivots, recost)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_fields(got, want, fields=("T", "d", "base", "phase", "pivots", "status", "x", "opt", "row")):
    """two reference dicts, or oracle.two_phase's dict against one, field by field and bit for bit"""
    for f in fields:
        g, w = got[f], want[f]
        if f in ("T", "d", "x", "row", "opt"):
            assert np.array_equal(bits(g), bits(w)), f
        elif f == "base":
            assert np.array_equal(g, w), f
        else:
            assert g == w, (f, g, w)


def state_tensors(states):
    """reference states of one shape -> a sx.BatchState on the GPU"""
    m, Ns = states[0]["T"].shape
    n = Ns - 1 - m
    cat = lambda f, dt: torch.from_numpy(np.stack([np.asarray(s[f], dtype=dt) for s in states])).cuda()  # noqa: E731
    return sx.BatchState(cat("T", np.float64), cat("d", np.float64), cat("base", np.int32), cat("phase", np.int32),
                         cat("pivots", np.int64), n, m)


def same_as_state_refs(out, refs, n, m, state=True):
    """a BatchTensors (with the objective row when the call asked for it) and its state against
    reference states, bit for bit: batch_refs.same_as_refs' fields, with NOT_ENDED handled by the
    caller, and T, d, base, phase and pivots of the state"""
    from batch_refs import same_as_refs

    same_as_refs(out, refs, n, m)
    if not state:
        return
    s = out.state
    assert s.n == n and s.m == m
    T, d, base = s.T.cpu().numpy(), s.d.cpu().numpy(), s.base.cpu().numpy()
    phase, pivots = s.phase.cpu().numpy(), s.pivots.cpu().numpy()
    B = len(refs)
    assert T.shape == (B, m, 1 + n + m) and d.shape == (B, 1 + n + 2 * m) and base.shape == (B, m)
    assert phase.shape == (B,) and phase.dtype == np.int32 and pivots.shape == (B, 2) and pivots.dtype == np.int64
    for k, ref in enumerate(refs):
        assert phase[k] == ref["phase"], k
        assert tuple(pivots[k]) == ref["pivots"], k
        assert np.array_equal(base[k], ref["base"]), k
        assert np.array_equal(bits(T[k]), bits(ref["T"])), k
        assert np.array_equal(bits(d[k]), bits(ref["d"])), k


# ---- the instances both test files use ----
SAVE_SHAPES = [(1, 1), (5, 4), (20, 10), (33, 31), (64, 64), (241, 64), (4, 513)]  # (n, m)
CAP_SHAPES = [(20, 10), (12, 9), (241, 64)]
CAPS = [1, 2, 8, 40, "p1", "p1+1"]
WARM_SHAPES = [(12, 10), (32, 16), (64, 64), (40, 60), (241, 64)]
WARM_SEEDS = range(1000, 1006)
WARM_SCALES = [0.01, 0.1, 1.0]
_INST = {}


def _once(key, make):
    if key not in _INST:
        _INST[key] = make()
    return _INST[key]


def save_instances(n, m):
    """three generated instances in [1, 100]"""
    return _once(("save", n, m), lambda: [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2, 3)])


def mixed_instances(n=12, m=9):
    """24 instances in [-100, 100]: FEASIBLE, UNBOUNDED and INFEASIBLE (phase-1 states) side by side"""
    return _once(("mixed", n, m),
                 lambda: [oracle.generate(n, m, s * 7919 + n * 100 + m, -100, 100) for s in range(1, 25)])


def cap_instances(n, m):
    return mixed_instances(n, m) if (n, m) == (12, 9) else save_instances(n, m)


def cap_value(cap, insts):
    """a cap of CAPS for one call: p1 is the phase-1 pivot count of the batch's first FEASIBLE
    instance, so that instance is capped exactly where phase 1 ends, or one selection later"""
    refs = [ref_state(*inst) for inst in insts]
    p1 = next(r for r in refs if r["status"] == oracle.FEASIBLE)["pivots"][0]
    return {"p1": p1, "p1+1": p1 + 1}.get(cap, cap)


def warm_instances(n, m):
    return _once(("warm", n, m), lambda: [oracle.generate(n, m, seed, 1, 100) for seed in WARM_SEEDS])


def warm_costs(c, seed, scale):
    """every cost perturbed by up to +-scale of itself"""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c))
    return c * (1.0 + scale * u)


def eviction_instances():
    """the four (20, 10) instances of test_gpu_batch_device.py::test_eviction"""
    return _once("evict", lambda: [oracle.generate(20, 10, seed, 1, 100) for seed in (2010, 3010, 4010, 5010)])


LADDER_CAPS = [1, 2, 8, 40]
STRUCTURED_FIRST_CAP = 3
MANY_CAP = 3
BAD_STATE_PHASE1_CAP = 2


def ladder_instances():
    """tie_ladders' B-small, whose pivots the lane tree decides in both phases, and two seed neighbours"""
    import tie_ladders as tl

    seed = tl.BATCH_CASES["B-small"][3]
    return _once("ladder", lambda: [tl.make_batch("B-small", seed + k) for k in range(3)])


def structured_instances(n, m):
    """the 22 structured_lps instances of one shape"""
    import structured_lps as slp

    return [inst for _, _, inst in slp.of_shape(n, m)]


def many_instances():
    """1,200 problems of (5, 4): more than the resident workgroups"""
    return _once("many", lambda: [oracle.generate(5, 4, 31 * s + 7, 1, 100) for s in range(1200)])


def bad_state_instances():
    """the batch of eight (20, 10) problems one of which gets a bad state"""
    return _once("bad", lambda: [oracle.generate(20, 10, 1000 * s + 2010, 1, 100) for s in range(1, 9)])
