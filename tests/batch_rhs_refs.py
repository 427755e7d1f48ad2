"""The re-solve of a kept batch state for a new right-hand side (simplex_solve_batch_device_rhs)
restated from the oracle's pieces -- argmin, ratio, gemv_partials, apply_update, and through
batch_state_refs._run build_phase1, update_objective and solve -- and nothing else, for
test_batch_rhs_host.py (the oracle alone) and test_gpu_batch_rhs.py (bit for bit against the GPU).

A reference state is batch_state_refs' dict; its phase may also be 3: phase 2's tableau inside the
dual loop (T, d and row as in phase 2, x zero and opt NaN).  A result that went through the dual loop
also says how many pivots that loop made in the call ("dual").
"""
import numpy as np

import oracle
from batch_state_refs import EPS, WARM_SEEDS, _negative, _once, _run, ref_resume, ref_state, save_instances

DBL_MAX = np.finfo(np.float64).max
NUMERIC_FAIL = -12


def _sum_partials(part):
    """block sums added left to right (orc_gemv_apply's order)"""
    s = part[0].copy()
    for k in range(1, part.shape[0]):
        s = s + part[k]
    return s


def new_rhs(state, b):
    """(S b, y b) of a phase-2 or phase-3 state: the right-hand-side column and the objective of the
    kept basis on b.  S is the stored slack block, y the slack entries of d; each sum is
    gemv_partials' (ascending by fma from +0.0 in 512-element blocks), the blocks added left to right"""
    T, d = state["T"], state["d"]
    m = T.shape[0]
    n = T.shape[1] - 1 - m
    b = np.ascontiguousarray(b, dtype=np.float64)
    St = np.ascontiguousarray(T[:, 1 + n:].T)  # rows k, columns i: p[i] = fma(S[i][k], b[k], p[i])
    col = _sum_partials(oracle.gemv_partials(St, b, m))
    y = np.ascontiguousarray(d[1 + n:1 + n + m].reshape(m, 1))
    obj = _sum_partials(oracle.gemv_partials(y, b, 1))[0]
    return col, obj


def dual_feasible(state):
    """the entering eps-argmin over d[1 .. Ns) does not compare below zero"""
    Ns = state["T"].shape[1]
    return not _negative(oracle.argmin(state["d"][1:Ns])[1])


def _dual(T, d, base, k0, max_pivots, argmin, enter_argmin=None, leave_argmin=None):
    """the dual loop on T [m, Ns], d [Ns], base, behind k0 pivots: (status or None when the loop was
    left, pivots); all three are written.  enter_argmin / leave_argmin: the selection of the entering
    ratio / of the leaving row alone (None: argmin)"""
    m, Ns = T.shape
    enter_argmin, leave_argmin = enter_argmin or argmin, leave_argmin or argmin
    k = k0
    while True:
        if max_pivots >= 0 and k >= max_pivots:
            return oracle.PIVOT_CAP, k
        r, bmin = leave_argmin(T[:, 0])
        if not _negative(bmin):
            return None, k
        neg = -T[r, 1:]
        if not (neg >= EPS).any():
            return oracle.INFEASIBLE, k
        e, _ = enter_argmin(np.array([oracle.ratio(d[1 + j], neg[j]) for j in range(Ns - 1)]))
        if e < 0 or e >= Ns - 1:
            return NUMERIC_FAIL, k
        prow, colE = T[r].copy(), T[:, 1 + e].copy()
        oracle.apply_update(T, d, prow, colE, r, prow[1 + e], d[1 + e])
        base[r] = e
        k += 1


def _enter_dual(T, d, base, pivots, c, max_pivots, argmin, enter_argmin=None, leave_argmin=None):
    """the dual loop at pivots[1], then phase 2 at the same count; T [m, Ns], d at full width"""
    m, Ns = T.shape
    n = Ns - 1 - m
    d2 = d[:Ns].copy()
    status, k = _dual(T, d2, base, pivots[1], max_pivots, argmin, enter_argmin, leave_argmin)
    d[:Ns] = d2
    d[Ns:] = 0.0
    if status is None:
        res = _run(T, d, base, 2, (pivots[0], k), c, max_pivots, False)
    else:
        res = {"T": T, "d": d, "base": base, "phase": 3, "pivots": (int(pivots[0]), int(k)), "status": status,
               "x": np.zeros(n), "opt": float("nan"), "row": d[:Ns].copy(), "art": None}
    res["dual"] = int(k - pivots[1])  # the dual loop's own pivots in this call
    return res


def ref_rhs(state, A, b, c, max_pivots=-1, argmin=oracle.argmin, enter_argmin=None, leave_argmin=None):
    """the state and results of a re-solve of `state` (left as it is) for the right-hand side b;
    argmin: the selection of the dual loop, the oracle's eps-argmin tree unless a test swaps it;
    enter_argmin / leave_argmin: one for the entering ratio / the leaving row alone (None: argmin)"""
    if state["phase"] == 1 or not dual_feasible(state):
        return ref_state(A, b, c, max_pivots)  # the cold start (shared: do not write it)
    T, d, base = state["T"].copy(), state["d"].copy(), state["base"].copy()
    T[:, 0], d[0] = new_rhs(state, b)
    return _enter_dual(T, d, base, (state["pivots"][0], 0), c, max_pivots, argmin, enter_argmin, leave_argmin)


def ref_rhs_resume(state, c, max_pivots=-1, argmin=oracle.argmin, enter_argmin=None, leave_argmin=None):
    """the plain resume (rerhs = 0): phases 1 and 2 are the state entry's, phase 3 re-enters the dual loop
    (argmin, enter_argmin, leave_argmin: that loop's selections, as in ref_rhs)"""
    if state["phase"] != 3:
        return ref_resume(state, c, max_pivots)
    return _enter_dual(state["T"].copy(), state["d"].copy(), state["base"].copy(), state["pivots"], c, max_pivots,
                       argmin, enter_argmin, leave_argmin)


# ---- the instances both test files use ----
RHS_SHAPES = [(1, 1), (5, 4), (20, 10), (33, 31), (64, 64), (241, 64), (4, 513), (600, 4)]  # (n, m)
RHS_SCALES = [0.1, 1.0]
HOST_SCALES = [0.01, 0.1, 1.0]
RHS_CAPS = [1, 2, 8]
CAP_SHAPE = (64, 64)  # every instance makes more than 8 dual pivots at scale 1.0
LADDER_SHAPE = (20, 10)
PHASE2_CAP_SHAPE, PHASE2_CAP = (600, 4), 6  # phase 1 ends within 6 pivots there, phase 2 does not


def rhs_instances(n, m):
    """three generated instances in [1, 100]; (600, 4) is not among batch_state_refs' shapes"""
    return save_instances(n, m)


def scaled_rhs(b, seed, scale):
    """every b_i moved by up to +-scale of itself (batch_state_refs.warm_costs' draw, on b)"""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(b))
    return b * (1.0 + scale * u)


def scaled_batch(insts, scale):
    """one new right-hand side per instance of a batch, drawn as warm_costs draws the costs: instance
    k with the seed WARM_SEEDS[0] + k"""
    return [scaled_rhs(inst[1], WARM_SEEDS[0] + k, scale) for k, inst in enumerate(insts)]


def negated_rhs(b, i):
    """b with b_i negated: on an instance in [1, 100] no x >= 0 satisfies row i"""
    b2 = b.copy()
    b2[i % len(b)] = -b2[i % len(b)]
    return b2


def ladder_cases():
    """[(instance, b')]: kept (20, 10) states whose new right-hand-side column S b' is, up to rounding
    far below eps / 4, a target t whose negative entries form an eps / 4 ladder -(1 + i eps / 4), so
    the leaving row depends on how the eps-argmin combines its candidates: the second instance with
    six entries at +1 in front of a descending ladder (ends FEASIBLE), the third with an ascending
    ladder on every row (ends INFEASIBLE after dual pivots)"""
    def make():
        n, m = LADDER_SHAPE
        cases = []
        for k, positive, descending in ((1, 6, True), (2, 0, False)):
            inst = rhs_instances(n, m)[k]
            lad = -(1.0 + np.arange(m - positive) * (EPS / 4))
            t = np.concatenate([np.full(positive, 1.0), lad[::-1] if descending else lad])
            cases.append((inst, np.linalg.solve(ref_state(*inst)["T"][:, 1 + n:], t)))
        return cases
    return _once("rhs-ladder", make)


def first_min(v):
    """np.argmin's selection: the first exact minimum, no eps"""
    i = int(np.argmin(v))
    return i, float(v[i])
