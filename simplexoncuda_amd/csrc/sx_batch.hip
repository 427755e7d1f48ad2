// sx_batch.hip -- batched solve: one 512-thread workgroup carries one whole LP
// through the two-phase method without a host round trip, then takes the next problem of the
// launch from a global work counter.  No workgroup ever waits for another: the only
// synchronisation is __syncthreads().
//
// Per problem the kernel performs, in order, exactly the operations of the serial restatement of
// the reference (oracle/simplex_oracle.c orc_two_phase): the same IEEE operations on the same
// operands and the reference's epsilon-argmin tree (sx_argmin.hpp) for both selections, so every
// result is bit-identical to twoPhaseMethodEx.  Compiled with -ffp-contract=off; every fused
// multiply-add is an explicit fma().
//
// The kernel is a template over where the working set (sx_common.hpp BatchLay) lives: dynamic LDS,
// or a per-workgroup slice of a device buffer.  The artificial column of row k stays bit-identical
// to its slack column (sx_common.hpp Cols), so T stores 1 + n + m columns and logical column
// j >= 1 + n + m reads stored column j - m; d keeps the full width.
//
// The two-phase method is written once (WG_TWO_PHASE and its parts), over a strided source (sx_common.hpp
// SxSource).  Its entries differ only in where a problem comes from and where its results go:
// k_batch_solve (simplex_solve_batch: ragged problems packed by the host -- column-major A, the
// source with A_sr = 1, A_sc = m -- results finished on the host), k_batch_solve_dev
// (simplex_solve_batch_device: one shape, the caller's strides, every result written by the kernel),
// k_batch_solve_rag (simplex_solve_batch_device_ragged: the same with per-problem dimensions
// inside one envelope shape), k_batch_solve_st (simplex_solve_batch_device_state: k_batch_solve_dev
// that can load a problem's working set from a saved state and write it to one), k_batch_solve_rhs
// (simplex_solve_batch_device_rhs: a saved state re-solved for a new right-hand side by the dual
// simplex, wg_dual, which shares its pivot, WG_PIVOT, with the primal loop), k_batch_solve_rows
// (simplex_solve_batch_device_rows: a saved state grown by new constraint rows, then the same dual loop),
// k_batch_solve_cols (simplex_solve_batch_device_cols: a saved state grown by new structural
// columns, then phase 2) and k_batch_solve_drop (simplex_solve_batch_device_drop: constraint rows or
// structural columns taken out of a saved state by forced pivots, then the same loops).  k_batch_solve_branch
// (simplex_solve_batch_device_branch) is k_batch_solve_rows for the children of a branch: many children per
// kept parent, the new bound row given as (variable, coefficient, right-hand side), no dense row read;
// k_batch_solve_cut (simplex_solve_batch_device_cut) is k_batch_solve_rows whose new rows are Gomory
// mixed-integer cuts that the kernel derives from the kept optimum and writes out for the caller.
// What surrounds the method is written once where that costs no time: every kernel names its static
// LDS through one WgScratch and draws its next problem with wg_next, and the two one-shape device
// entries end with the same epilogue, wg_write_results, which writes a problem's results into the
// caller's dense arrays; k_batch_solve_rag keeps that epilogue written out over its envelope.  The five
// kernels on a saved state share their head, the state's tests, the cold start, the loops behind the
// front and the end (WG_KEPT_HEAD .. WG_KEPT_END), so each shows only its own front.

#include <float.h>

#include "sx_argmin.hpp"
#include "sx_common.hpp"

namespace {

#define SX_EVICTED (-100)  // phase result inside the kernel: the resident budget ran out

struct BatchWork {
    double *T, *d, *prow, *colE;
    TilePart *parts;
    int *base;
    int n, m, ld;
};

// The kernels' static LDS: the reduction scratch of block_argmin512 / stage2_512, the argmin's result
// and the work counter's value.  WG_SCRATCH declares them in a kernel and names them through one
// WgScratch, which is what wg_next, wg_argmin, wg_solve and the macros take.  They stay five
// __shared__ objects: as members of one object the address of i[] is derived from that of v[] in
// every reduction step, and k_batch_solve measured 1.3-2 % slower.
struct WgScratch {
    double *v;  // [16]
    int *i;     // [16]
    double &rv;
    int &ri;
    unsigned &k;
};
#define WG_SCRATCH(sc)          \
    __shared__ double s_v[16];  \
    __shared__ int s_i[16];     \
    __shared__ double s_rv;     \
    __shared__ int s_ri;        \
    __shared__ unsigned s_k;    \
    const WgScratch sc { s_v, s_i, s_rv, s_ri, s_k }

// the launch's next problem: thread 0 draws the work counter, every thread gets the value
__device__ __forceinline__ unsigned wg_next(unsigned *counter, const WgScratch &sc) {
    if (threadIdx.x == 0) sc.k = atomicAdd(counter, 1u);
    __syncthreads();
    return sc.k;
}

// orc_argmin over val(0) .. val(L - 1): per 512-wide tile the per-thread grid-stride pre-combine and
// block_argmin512, then pass 2 over the tile winners when there is more than one tile.  The
// workgroup walks the tiles one after the other.  Result in every thread.
template <class F>
__device__ __forceinline__ void wg_argmin(int L, F val, TilePart *parts, const WgScratch &sc, double &v_out, int &i_out) {
    const int tiles = L > SX_TILE ? (L + SX_TILE - 1) / SX_TILE : 1;
    for (int b = 0; b < tiles; ++b) {
        double v = DBL_MAX;
        int i = -1;
        for (int idx = b * SX_TILE + (int)threadIdx.x; idx < L; idx += SX_TILE * tiles) {
            const double c = val(idx);
            if (cmp_eps(c, v) < 0) {
                v = c;
                i = idx;
            }
        }
        block_argmin512(v, i, sc.v, sc.i);
        if (threadIdx.x == 0) {
            if (tiles == 1) {
                sc.rv = v;
                sc.ri = i;
            } else {
                parts[b].v = v;
                parts[b].idx = i;
                parts[b].elig = 0;
            }
        }
        __syncthreads();
    }
    if (tiles > 1) {
        double v;
        int i;
        stage2_512(parts, tiles, v, i, sc.v, sc.i);
        if (threadIdx.x == 0) {
            sc.rv = v;
            sc.ri = i;
        }
        __syncthreads();
    }
    v_out = sc.rv;
    i_out = sc.ri;
}

// orc_update_objective at width N: coef[i] = d[1 + base[i]] snapshot (kept in colE), then per column
// the 512-row block partials from 0.0 in ascending row order, added left to right, d[j] -= s.
__device__ __forceinline__ void wg_update_objective(const BatchWork &w, int N) {
    const int art0 = 1 + w.n + w.m;
    for (int i = threadIdx.x; i < w.m; i += SX_TILE) w.colE[i] = w.d[1 + w.base[i]];
    __syncthreads();
    for (int j = threadIdx.x; j < N; j += SX_TILE) {
        const double *col = w.T + (j >= art0 ? j - w.m : j);
        double s = 0.0;
        for (int i0 = 0; i0 < w.m; i0 += SX_TILE) {
            const int i1 = i0 + SX_TILE < w.m ? i0 + SX_TILE : w.m;
            double p = 0.0;
            for (int i = i0; i < i1; ++i) p = fma(col[(size_t)i * w.ld], w.colE[i], p);
            s = i0 == 0 ? p : s + p;
        }
        w.d[j] = w.d[j] - s;
    }
    __syncthreads();
}

// orc_apply_update with the basis change, the pivot of the primal loop (wg_solve) and of the dual
// loop (wg_dual), written once: row r leaves, variable e (stored column ce) enters, colE holds the
// entering column and d_e is the entering variable's entry of d (N wide).  The pivot-row copy and the
// row factors -(a_ie / p) first -- T is not written before the barrier -- then the row sweep and d.
// Ends behind a barrier.  Expanded in both loops, which declare w, m, ld, Ns, art0 and the sweep's
// lane grouping (WG_ROW_LANES), and not a function: as one, inlined, it leaves wg_solve's
// instructions in the four earlier kernels other than they were.
#define WG_ROW_LANES()                                                                               \
    /* the row update gives each row to 16, 32 or 64 consecutive lanes (a row sweep by consecutive */ \
    /* lanes is conflict-free at any stride; narrow tableaux keep more rows in flight) */            \
    const int g = Ns <= 16 ? 4 : Ns <= 32 ? 5 : 6;                                                   \
    const int G = 1 << g, RP = SX_TILE >> g;                                                         \
    const int rl = (int)threadIdx.x >> g, cl = (int)threadIdx.x & (G - 1)
#define WG_PIVOT(N, r, e, ce, d_e)                                                                              \
    do {                                                                                                        \
        const double *rowr = w.T + (size_t)r * ld;                                                              \
        const double p = rowr[ce];                                                                              \
        for (int j = threadIdx.x; j < Ns; j += SX_TILE) w.prow[j] = rowr[j];                                    \
        for (int i = threadIdx.x; i < m; i += SX_TILE) w.colE[i] = -w.colE[i] / p;                              \
        if (threadIdx.x == 0) w.base[r] = e;                                                                    \
        __syncthreads();                                                                                        \
        for (int i = rl; i < m; i += RP) {                                                                      \
            double *row = w.T + (size_t)i * ld;                                                                 \
            if (i == r) {                                                                                       \
                for (int j = cl; j < Ns; j += G) row[j] = w.prow[j] / p;                                        \
            } else {                                                                                            \
                const double f = w.colE[i];                                                                     \
                for (int j = cl; j < Ns; j += G) row[j] = fma(f, w.prow[j], row[j]);                            \
            }                                                                                                   \
        }                                                                                                       \
        const double fd = -d_e / p;                                                                             \
        for (int j = threadIdx.x; j < N; j += SX_TILE) w.d[j] = fma(fd, w.prow[j >= art0 ? j - m : j], w.d[j]); \
        __syncthreads();                                                                                        \
    } while (0)

// orc_solve at width N, continued behind k0 pivots of the phase: pivots until the phase ends, the cap
// on the phase's total is reached (SX_PIVOT_CAP) or one more pivot would exceed the resident budget
// of this call, `budget` pivots behind k0 (SX_EVICTED).  That test sits behind the stop and unbounded
// tests and in front of the first write to T, d or base, so an eviction leaves what a cap at the
// same count leaves.  A fresh solve passes the literal 0 for k0.  Uniform over the workgroup.
__device__ __forceinline__ int wg_solve(const BatchWork &w, int N, long long max_pivots, long long budget,
                                        long long k0, long long &pivots, const WgScratch &sc) {
    const int n = w.n, m = w.m, ld = w.ld, Ns = 1 + n + m, art0 = Ns;
    WG_ROW_LANES();
    long long k = k0;
    for (;;) {
        if (max_pivots >= 0 && k >= max_pivots) {
            pivots = k;
            return SX_PIVOT_CAP;
        }
        double dmin;
        int e;
        wg_argmin(N - 1, [&](int idx) { return w.d[1 + idx]; }, w.parts, sc, dmin, e);
        if (!(cmp_eps(dmin, 0.0) < 0)) {
            pivots = k;
            return SX_FEASIBLE;
        }
        const int ce = 1 + e >= art0 ? 1 + e - m : 1 + e;  // stored column of the entering variable
        int any = 0;
        for (int i = threadIdx.x; i < m; i += SX_TILE) {
            const double a = w.T[(size_t)i * ld + ce];
            w.colE[i] = a;
            any |= a >= SX_EPS;
        }
        any = __syncthreads_or(any);
        if (!any) {
            pivots = k;
            return SX_UNBOUNDED;
        }
        if (k - k0 >= budget) {
            pivots = k;
            return SX_EVICTED;
        }
        double rv;
        int r;
        wg_argmin(
            m,
            [&](int i) {
                const double a = w.colE[i], b = w.T[(size_t)i * ld];
                return cmp_eps(a, 0.0) > 0 ? b / a : DBL_MAX;
            },
            w.parts, sc, rv, r);
        if (r < 0 || r >= m) {
            pivots = k;
            return SX_NUMERIC_FAIL;
        }
        WG_PIVOT(N, r, e, ce, dmin);
        ++k;
    }
}

// The dual simplex on phase 2's tableau (width Ns = 1 + n + m), continued behind k0 pivots: the row of
// the most negative RHS entry leaves (the reference's eps-argmin tree over T[i][0]), the entering
// variable is the eps-argmin of d[1 + j] / -T[r][1 + j] over the columns with compare(-T[r][1 + j], 0)
// > 0, and the pivot is the primal loop's (WG_PIVOT).  The objective row stays dual feasible; the
// loop is left (SX_FEASIBLE: the tableau is primal feasible, phase 2 follows) when no RHS entry
// compares below zero.  Ends inside the loop with SX_PIVOT_CAP, SX_INFEASIBLE (a negative RHS entry
// whose row has no entry <= -eps: the row cannot be satisfied), SX_EVICTED -- wg_solve's place: behind
// the stop tests, in front of the first write -- or SX_NUMERIC_FAIL.  Uniform over the workgroup.
__device__ __forceinline__ int wg_dual(const BatchWork &w, long long max_pivots, long long budget, long long k0,
                                       long long &pivots, const WgScratch &sc) {
    const int m = w.m, ld = w.ld, Ns = 1 + w.n + m, art0 = Ns;
    WG_ROW_LANES();
    long long k = k0;
    for (;;) {
        if (max_pivots >= 0 && k >= max_pivots) {
            pivots = k;
            return SX_PIVOT_CAP;
        }
        double bmin;
        int r;
        wg_argmin(m, [&](int i) { return w.T[(size_t)i * ld]; }, w.parts, sc, bmin, r);
        if (!(cmp_eps(bmin, 0.0) < 0)) {
            pivots = k;
            return SX_FEASIBLE;
        }
        if (r < 0 || r >= m) {  // (a value that compares below zero has an index; the row is indexed with it)
            pivots = k;
            return SX_NUMERIC_FAIL;
        }
        const double *lrow = w.T + (size_t)r * ld;
        int any = 0;
        for (int j = 1 + (int)threadIdx.x; j < Ns; j += SX_TILE) any |= -lrow[j] >= SX_EPS;
        any = __syncthreads_or(any);
        if (!any) {
            pivots = k;
            return SX_INFEASIBLE;
        }
        if (k - k0 >= budget) {
            pivots = k;
            return SX_EVICTED;
        }
        double rv;
        int e;
        wg_argmin(
            Ns - 1,
            [&](int idx) {
                const double a = -lrow[1 + idx];
                return cmp_eps(a, 0.0) > 0 ? w.d[1 + idx] / a : DBL_MAX;
            },
            w.parts, sc, rv, e);
        if (e < 0 || e >= Ns - 1) {
            pivots = k;
            return SX_NUMERIC_FAIL;
        }
        const int ce = 1 + e;
        const double d_e = w.d[ce];
        for (int i = threadIdx.x; i < m; i += SX_TILE) w.colE[i] = w.T[(size_t)i * ld + ce];
        WG_PIVOT(Ns, r, e, ce, d_e);
        ++k;
    }
}

// the working set at W (sx_common.hpp BatchLay) of a problem of n variables and m constraints
__device__ __forceinline__ BatchWork wg_carve(double *W, int n, int m) {
    const BatchLay lay = sx_batch_lay(n, m);
    BatchWork w;
    w.T = W;
    w.d = W + lay.d;
    w.prow = W + lay.prow;
    w.colE = W + lay.colE;
    w.parts = reinterpret_cast<TilePart *>(W + lay.parts);
    w.base = reinterpret_cast<int *>(W + lay.base);
    w.n = n;
    w.m = m;
    w.ld = lay.ld;
    return w;
}

// consecutive lanes walk A's faster-varying dimension
__device__ __forceinline__ bool wg_by_col(const SxSource &src) {
    return (src.A_sc < 0 ? -src.A_sc : src.A_sc) <= (src.A_sr < 0 ? -src.A_sr : src.A_sr);
}

// orc_build_phase1 of the problem at src: RHS, A, slack (the artificial block aliases it); a row with
// compare(b_i) < 0 is negated across all its entries, zeros included.  Consecutive lanes walk A's
// faster-varying dimension: the same copies and negations in either walk.  Ends behind a barrier.
__device__ __forceinline__ void wg_build(const BatchWork &w, const SxSource &src, bool by_col) {
    const int n = w.n, m = w.m, ld = w.ld;
    const auto structural = [&](int i, int j) {
        const double v = src.A[(long long)i * src.A_sr + (long long)j * src.A_sc];
        w.T[(size_t)i * ld + 1 + j] = cmp_eps(src.b[(long long)i * src.b_si], 0.0) < 0 ? -v : v;
    };
    if (by_col) {
        for (int x = threadIdx.x; x < n * m; x += SX_TILE) structural(x / n, x % n);
    } else {
        for (int x = threadIdx.x; x < n * m; x += SX_TILE) structural(x % m, x / m);
    }
    for (int x = threadIdx.x; x < m * (m + 1); x += SX_TILE) {
        const int i = x / (m + 1), t = x - i * (m + 1);
        const double b = src.b[(long long)i * src.b_si];
        const double v = t == 0 ? b : (t - 1 == i ? 1.0 : 0.0);
        w.T[(size_t)i * ld + (t == 0 ? 0 : n + t)] = cmp_eps(b, 0.0) < 0 ? -v : v;
    }
    for (int j = threadIdx.x; j < 1 + n + 2 * m; j += SX_TILE) w.d[j] = j <= n + m ? 0.0 : 1.0;
    for (int i = threadIdx.x; i < m; i += SX_TILE) w.base[i] = n + m + i;
    __syncthreads();
}

// what phase 1 decided, given its wg_solve result: SX_FEASIBLE means phase 2 follows
__device__ __forceinline__ int wg_classify(const BatchWork &w, int st1) {
    const int n = w.n, m = w.m;
    if (st1 == SX_PIVOT_CAP || st1 == SX_NUMERIC_FAIL || st1 == SX_EVICTED) return st1;
    if (cmp_eps(w.d[0], 0.0) < 0) return SX_INFEASIBLE;
    int art = 0;
    for (int i = threadIdx.x; i < m; i += SX_TILE) art |= w.base[i] >= n + m && w.base[i] < n + 2 * m;
    return __syncthreads_or(art) ? SX_DEGENERATE : SX_FEASIBLE;
}

// phase 2's row: costs -c, slack costs 0, d[0] kept.  Ends behind a barrier.
__device__ __forceinline__ void wg_phase2_costs(const BatchWork &w, const SxSource &src) {
    for (int j = threadIdx.x; j < w.n; j += SX_TILE) w.d[1 + j] = -src.c[(long long)j * src.c_sj];
    for (int j = threadIdx.x; j < w.m; j += SX_TILE) w.d[1 + w.n + j] = 0.0;
    __syncthreads();
}

struct TwoPhase {
    int status;  // SX_EVICTED included
    bool ph2;    // phase 2 was entered: d holds its row on [0, 1 + n + m), stale phase-1 values behind it
    long long p1, p2;
};

// orc_two_phase of the problem at src in the working set w, into the TwoPhase t; sc is the
// kernel's WgScratch.  Every path ends behind a barrier, so T, d and base are
// complete afterwards.  Uniform over the workgroup.  Expanded in the kernel's body and not a
// function: the workgroup size inside the three __syncthreads_or of a problem is folded to the
// launch's only where they reach the kernel as three separate sites.
// Its two parts are entry points of their own for a saved state (k_batch_solve_st), which passes
// the pivots a phase has behind it where the fresh solve passes the literal 0, which folds away:
// WG_PHASE1 -- phase 1 at width N1 on a row that is already canonical, and what it decided;
#define WG_PHASE1(t, w, N1, max_pivots, budget, k1, sc)                                      \
    do {                                                                                     \
        (t).status = wg_classify(w, wg_solve(w, N1, max_pivots, budget, k1, (t).p1, sc));    \
        (t).ph2 = (t).status == SX_FEASIBLE;                                                 \
    } while (0)
// WG_PHASE2 -- phase 2 at width Ns on a canonical row.
#define WG_PHASE2(t, w, Ns, max_pivots, budget, k2, sc) \
    (t).status = wg_solve(w, Ns, max_pivots, budget, k2, (t).p2, sc)
#define WG_TWO_PHASE(t, w, src, by_col, max_pivots, budget, sc)        \
    do {                                                               \
        const int Ns_ = 1 + (w).n + (w).m, N1_ = Ns_ + (w).m;          \
        wg_build(w, src, by_col);                                      \
        wg_update_objective(w, N1_);                                   \
        (t).p1 = (t).p2 = 0;                                           \
        WG_PHASE1(t, w, N1_, max_pivots, budget, 0LL, sc);             \
        if ((t).ph2) {                                                 \
            wg_phase2_costs(w, src);                                   \
            wg_update_objective(w, Ns_);                               \
            WG_PHASE2(t, w, Ns_, max_pivots, budget, 0LL, sc);         \
        }                                                              \
    } while (0)

// The one-shape device entries' epilogue (k_batch_solve_dev, k_batch_solve_st): problem k's results,
// from the working set w and what the two-phase method left in t, into the caller's dense arrays
// (BatchDevArgs), so nothing is left for the host.  A problem that failed its kernel's device-side
// test (!good) has every output cleared.  Only __syncthreads() inside, so this is a function; it
// ends without a barrier.  (k_batch_solve_rag keeps its own, over the envelope: DESIGN.md §10.2.)
__device__ __forceinline__ void wg_write_results(const BatchDevArgs &a, const BatchWork &w, const TwoPhase &t, size_t k,
                                                 bool good) {
    const int n = w.n, m = w.m, Ns = 1 + n + m, N1 = Ns + m;
    const bool feasible = t.status == SX_FEASIBLE, evicted = t.status == SX_EVICTED;
    if (a.x != nullptr) {
        // getSolutionHost, staged in the pivot-row copy (1 + n + m >= n doubles, free by now):
        // zeros, then x[base[i]] = T[i][0] for the basic variables, written out by consecutive lanes
        for (int j = threadIdx.x; j < n; j += SX_TILE) w.prow[j] = 0.0;
        __syncthreads();
        if (feasible)
            for (int i = threadIdx.x; i < m; i += SX_TILE) {
                const unsigned bi = (unsigned)w.base[i];
                if (bi < (unsigned)n) w.prow[bi] = w.T[(size_t)i * w.ld];
            }
        __syncthreads();
        double *x = a.x + k * (size_t)n;
        for (int j = threadIdx.x; j < n; j += SX_TILE) x[j] = w.prow[j];
    }
    if (a.base != nullptr) {
        int *base_out = a.base + k * (size_t)m;
        for (int i = threadIdx.x; i < m; i += SX_TILE) base_out[i] = good ? w.base[i] : -1;
    }
    // the row simplex_last_objective_row reports: phase 2's 1 + n + m entries once phase 2 was
    // entered (what lies behind them in d is stale phase-1 data), else phase 1's full width;
    // nothing of an evicted or cleared problem
    const int width = evicted || !good ? 0 : t.ph2 ? Ns : N1;
    if (a.objrow != nullptr) {
        double *row = a.objrow + k * (size_t)N1;
        for (int j = threadIdx.x; j < N1; j += SX_TILE) row[j] = j < width ? w.d[j] : 0.0;
    }
    if (threadIdx.x == 0) {
        a.status[k] = evicted ? SX_NOT_ENDED : t.status;
        a.pivots[2 * k] = t.p1;
        a.pivots[2 * k + 1] = t.p2;
        a.opt[k] = feasible ? w.d[0] : __builtin_nan("");
        if (a.row_width != nullptr) a.row_width[k] = width;
        if (evicted) atomicAdd(a.evicted, 1);
    }
}

// The stored columns of a saved tableau, dense at T_in with stride Ns0 (cells0 of them), into the
// working set wk, whose shape may be another: re-packed to wk's odd ld by consecutive lanes, which walk
// the dense rows.  No barrier.
__device__ __forceinline__ void wg_load_T(const BatchWork &wk, const double *T_in, int Ns0, int cells0) {
    for (int x = threadIdx.x; x < cells0; x += SX_TILE) {
        const int i = x / Ns0;
        wk.T[(size_t)i * wk.ld + (x - i * Ns0)] = T_in[x];
    }
}

// A saved state (sx_common.hpp BatchState) of problem k into the working set of the same shape: the
// stored columns of T (wg_load_T) and d at full width.  The basis is loaded by the kernels, through
// their range test (WG_STATE_TEST).  No barrier.  This and WG_STORE_STATE are expanded in the
// kept-state kernels, which declare w, k, m, Ns, N1 and cells; as functions they leave
// k_batch_solve_st's instructions other than they were.
#define WG_LOAD_STATE(in)                                                 \
    do {                                                                  \
        wg_load_T(w, (in).T + (size_t)k * (size_t)cells, Ns, cells);      \
        const double *d_in = (in).d + (size_t)k * (size_t)N1;             \
        for (int j = threadIdx.x; j < N1; j += SX_TILE) w.d[j] = d_in[j]; \
    } while (0)
// ... and the working set into a state (nothing when out.T is null) with its phase, `ph`; of a problem
// that failed its kernel's tests (!good) only phase 0 is written.  What phase 2 leaves behind its row
// in d is stale phase-1 data and is not kept.
#define WG_STORE_STATE(out, t, good, ph)                                                                            \
    do {                                                                                                            \
        if ((out).T != nullptr) {                                                                                   \
            if (good) {                                                                                             \
                double *T_out = (out).T + (size_t)k * (size_t)cells;                                                \
                for (int x = threadIdx.x; x < cells; x += SX_TILE) {                                                \
                    const int i = x / Ns;                                                                           \
                    T_out[x] = w.T[(size_t)i * w.ld + (x - i * Ns)];                                                \
                }                                                                                                   \
                double *d_out = (out).d + (size_t)k * (size_t)N1;                                                   \
                for (int j = threadIdx.x; j < N1; j += SX_TILE) d_out[j] = (t).ph2 && j >= Ns ? 0.0 : w.d[j];       \
                int *base_out = (out).base + (size_t)k * (size_t)m;                                                 \
                for (int i = threadIdx.x; i < m; i += SX_TILE) base_out[i] = w.base[i];                             \
            }                                                                                                       \
            if (threadIdx.x == 0) {                                                                                 \
                (out).phase[k] = ph;                                                                                \
                if (good) {                                                                                         \
                    (out).pivots[2 * (size_t)k] = (t).p1;                                                           \
                    (out).pivots[2 * (size_t)k + 1] = (t).p2;                                                       \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
    } while (0)

// What the kernels on a kept state share (k_batch_solve_st, _rhs, _rows, _cols, _drop, _branch, _cut),
// written once; each kernel keeps its own front: how the in-state is embedded into the working set and
// what makes the tableau canonical again -- of which the three that grow the state by rows (_rows,
// _branch, _cut) share the embedding and the reduction of a new row (WG_GROWN_ROW, WG_LOAD_GROWN,
// WG_REDUCE_ROW) and keep where a new row comes from.  All but the dense load (wg_load_T) are macros,
// expanded in the kernel's body, which declares a, sc, w, src, k and the names of the head: as
// functions, and even with the head's declarations in another order, they leave the kernels'
// instructions other than they were.
//
// WG_KEPT_HEAD -- the kernel's head, in two parts with the in-state's shape between them: the static
// and dynamic LDS, the working set W and the call's shape with its widths; then (WG_KEPT_CARVE) the
// carve w, behind it MORE (k_batch_solve_drop's second carve; else empty), the resident budget and
// wg_by_col's rule, decided once because the strides are the launch's.
#define WG_KEPT_HEAD(a, sc)                                                                               \
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];                                        \
    WG_SCRATCH(sc);                                                                                       \
    double *const W = LDS ? s_dyn : (a).ws + (size_t)blockIdx.x * (size_t)(a).slice;                      \
    const int n = (a).n, m = (a).m, Ns = 1 + n + m, N1 = Ns + m
#define WG_KEPT_CARVE(a, MORE)                                                                            \
    const BatchWork w = wg_carve(W, n, m);                                                                \
    MORE;                                                                                                 \
    const long long budget = (a).budget > 0 ? (a).budget : sx_batch_default_budget(n, m);                 \
    const bool by_col = ((a).A_sc < 0 ? -(a).A_sc : (a).A_sc) <= ((a).A_sr < 0 ? -(a).A_sr : (a).A_sr)

// WG_STATE_TEST -- the in-state of problem sk (the kernel's k, but for k_batch_solve_branch's parent),
// shape (n0, m0), tested before anything is indexed with it: the phase (PH_OK, an expression in ph),
// both pivot counts >= 0, then the basis, which indexes d (and, through the alias, T), so phase 2 knows
// no artificial variable.  Declares ph, q1, q2; the result is the kernel's `good`, which GOOD declares
// (`bool good`) or names (k_batch_solve_st's).  The basis is loaded on the way: ROW is the statement for
// row i < rows, which reads base_in[i], stores the working set's entry and ors an entry outside
// [0, lim) into bad (WG_BASE_ROW: the entry as it is; WG_GROWN_ROW: the in-state's m0 entries tested
// against its own range -- what is valid only for the grown shape is refused --, behind them the new
// rows' slacks, which are basic); MORE is a further statement that ors into bad.  Ends behind a barrier.
#define WG_BASE_ROW(wk)                 \
    {                                   \
        const int bi = base_in[i];      \
        (wk).base[i] = bi;              \
        bad |= (unsigned)bi >= lim;     \
    }
#define WG_GROWN_ROW(wk, m0)                                                                         \
    {                                                                                                \
        const int bi = i < (m0) ? base_in[i] : n + i; /* a new row's slack is basic */               \
        (wk).base[i] = bi;                                                                           \
        bad |= i < (m0) && (unsigned)bi >= lim;                                                      \
    }
#define WG_STATE_TEST(GOOD, in, sk, PH_OK, n0, m0, rows, ROW, MORE)                                  \
    const int ph = (in).phase[sk];                                                                   \
    const long long q1 = (in).pivots[2 * (size_t)(sk)], q2 = (in).pivots[2 * (size_t)(sk) + 1];      \
    GOOD = (PH_OK) && q1 >= 0 && q2 >= 0;                                                            \
    WG_STATE_BASIS(in, sk, n0, m0, rows, ROW, MORE)
// ... and its second half alone, the basis, for the kernel that has ph and `good` by then
// (k_batch_solve_branch, which must range-test sk before it reads the phase and the counts).
#define WG_STATE_BASIS(in, sk, n0, m0, rows, ROW, MORE)                                              \
    if (good) {                                                                                      \
        const unsigned lim = ph == 1 ? (unsigned)((n0) + 2 * (m0)) : (unsigned)((n0) + (m0));        \
        const int *base_in = (in).base + (size_t)(sk) * (size_t)(m0);                                \
        int bad = 0;                                                                                 \
        for (int i = threadIdx.x; i < (rows); i += SX_TILE) ROW                                      \
        MORE                                                                                         \
        good = !__syncthreads_or(bad);                                                               \
    }

// WG_LOAD_GROWN -- the in-state of problem sk, shape (n, m0 = m - q), into the working set of the shape
// grown by q rows, for the kernels that declare m0, Ns0, N10 and cells0 beside the head's names: the
// dense in-state is walked at its stride Ns0 into the grown shape's odd ld (wg_load_T), old rows end in
// q entries of +0.0 (the new slack columns), d ends in +0.0 from Ns0 on.  The basis, with the new rows'
// basic slacks, is WG_STATE_TEST's with WG_GROWN_ROW.  Ends behind a barrier.
#define WG_LOAD_GROWN(in, sk, q)                                                                     \
    do {                                                                                             \
        wg_load_T(w, (in).T + (size_t)(sk) * (size_t)cells0, Ns0, cells0);                           \
        for (int x = threadIdx.x; x < m0 * (q); x += SX_TILE) {                                      \
            const int i = x / (q);                                                                   \
            w.T[(size_t)i * w.ld + Ns0 + (x - i * (q))] = 0.0;                                       \
        }                                                                                            \
        const double *d_in = (in).d + (size_t)(sk) * (size_t)N10;                                    \
        for (int j = threadIdx.x; j < N1; j += SX_TILE) w.d[j] = j < Ns0 ? d_in[j] : 0.0;            \
        __syncthreads();                                                                             \
    } while (0)

// WG_REDUCE_ROW -- new row r of a grown working set reduced against the kept basis, a row operation
// on the grown system.  Declares row = T[r]; the multipliers f_i = MULT (an
// expression with i and bi = base[i] in scope: the raw row's entry in the column of old row i's basic
// variable, +0.0 for a basic slack) are staged once in colE (m >= m0 doubles, free by then); behind a
// barrier consecutive lanes take consecutive columns j -- the reads of T[i][j] are row-contiguous --
// and row[j] = RAW (an expression with j and row in scope: the raw row's entry), then
// fma(-f_i, T[i][j], .) for i = 0 .. m0 - 1 in that order.  Ends behind a barrier: colE may be
// rewritten for the next row, and T is complete behind the last.
#define WG_REDUCE_ROW(r, MULT, RAW)                                                                  \
    do {                                                                                             \
        double *row = w.T + (size_t)(r) * w.ld;                                                      \
        for (int i = threadIdx.x; i < m0; i += SX_TILE) {                                            \
            const int bi = w.base[i];                                                                \
            w.colE[i] = MULT;                                                                        \
        }                                                                                            \
        __syncthreads();                                                                             \
        for (int j = threadIdx.x; j < Ns; j += SX_TILE) {                                            \
            double acc = RAW;                                                                        \
            for (int i = 0; i < m0; ++i) acc = fma(-w.colE[i], w.T[(size_t)i * w.ld + j], acc);      \
            row[j] = acc;                                                                            \
        }                                                                                            \
        __syncthreads();                                                                             \
    } while (0)

// WG_DUAL_LOST -- is the row d of the carve wk, N wide, no longer dual feasible?  wg_solve's entering
// selection and stop test, into `lost`.
#define WG_DUAL_LOST(lost, wk, N)                                                                    \
    do {                                                                                             \
        double dmin;                                                                                 \
        int e;                                                                                       \
        wg_argmin((N) - 1, [&](int idx) { return (wk).d[1 + idx]; }, (wk).parts, sc, dmin, e);       \
        lost = cmp_eps(dmin, 0.0) < 0;                                                               \
    } while (0)

// WG_SLACK_DOT -- into the new double `s`: row i of the slack block (row m: the slack entries of d)
// times the m doubles staged in the pivot-row copy, S[i][.] v or y v: per element the chain of
// wg_update_objective (512-element blocks from +0.0 by fma, added left to right).  Consecutive lanes
// take consecutive rows: the odd ld keeps the gather conflict-free.  Declares row as well.
#define WG_SLACK_DOT(s, i)                                                            \
    const double *row = ((i) < m ? w.T + (size_t)(i) * w.ld : w.d) + 1 + n;           \
    double s = 0.0;                                                                   \
    for (int k0 = 0; k0 < m; k0 += SX_TILE) {                                         \
        const int k1 = k0 + SX_TILE < m ? k0 + SX_TILE : m;                           \
        double u = 0.0;                                                               \
        for (int kk = k0; kk < k1; ++kk) u = fma(row[kk], w.prow[kk], u);             \
        s = k0 == 0 ? u : s + u;                                                      \
    }

// WG_COLD_START -- the problem is built from A, b, c and solved as k_batch_solve_dev does, at the
// sites every path shares: phase 1's tableau and canonical row, no pivot behind it.  BUILD is the
// kernel's build of the working set, wg_build(...) or, of a composite problem, wg_build_branch(...).
#define WG_COLD_START(t, dual, BUILD)    \
    do {                                 \
        BUILD;                           \
        wg_update_objective(w, N1);      \
        (t).p1 = (t).p2 = 0;             \
        (t).ph2 = dual = false;          \
    } while (0)

// WG_KEPT_TAIL -- the loops behind every front, from where t and `dual` (the problem stands inside the
// dual loop) say the problem stands: phase 1 behind t.p1 and phase 2's costs, or the dual loop behind
// t.p2, then phase 2 at the same count.  What ends inside the dual loop leaves `dual` set.
#define WG_KEPT_TAIL(t, dual)                                                          \
    do {                                                                               \
        if (!(t).ph2) {                                                                \
            WG_PHASE1(t, w, N1, a.max_pivots, budget, (t).p1, sc);                     \
            if ((t).ph2) {                                                             \
                wg_phase2_costs(w, src);                                               \
                wg_update_objective(w, Ns);                                            \
                (t).p2 = 0;                                                            \
            }                                                                          \
        }                                                                              \
        if ((t).ph2 && dual) {                                                         \
            (t).status = wg_dual(w, a.max_pivots, budget, (t).p2, (t).p2, sc);         \
            dual = (t).status != SX_FEASIBLE;                                          \
        }                                                                              \
        if ((t).ph2 && !dual) WG_PHASE2(t, w, Ns, a.max_pivots, budget, (t).p2, sc);   \
    } while (0)

// WG_KEPT_END -- the device entry's epilogue, then the working set into a.out (which may be a.in: the
// workgroup has loaded all of its problem by then).  A problem whose state failed the tests (!good)
// has every output cleared and phase 0; what ended inside the dual loop is saved as phase 3.
#define WG_KEPT_END(t, good, dual)                                                   \
    do {                                                                             \
        wg_write_results(a, w, t, k, good);                                          \
        WG_STORE_STATE(a.out, t, good, !(good) ? 0 : (dual) ? 3 : (t).ph2 ? 2 : 1);  \
    } while (0)

// simplex_solve_batch: ragged problems packed by the host (A column-major, then b, then c), the RHS
// column, the basis and a BatchRes per problem written out for the host to finish.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE) void k_batch_solve(BatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    WG_SCRATCH(sc);
    double *const W = LDS ? s_dyn : a.ws + (size_t)blockIdx.x * (size_t)a.slice;
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const int id = a.order[k];
        const BatchProb pb = a.probs[id];
        const int n = pb.n, m = pb.m;
        const BatchWork w = wg_carve(W, n, m);
        const double *A = a.in + pb.in_off, *bv = A + (size_t)n * m;
        const SxSource src{A, 1, m, bv, 1, bv + m, 1};
        const long long budget = a.budget > 0 ? a.budget : sx_batch_default_budget(n, m);
        TwoPhase t;
        WG_TWO_PHASE(t, w, src, wg_by_col(src), a.max_pivots, budget, sc);
        double *out = a.out + pb.out_off;
        int *base_out = reinterpret_cast<int *>(out + m);
        for (int i = threadIdx.x; i < m; i += SX_TILE) {
            out[i] = w.T[(size_t)i * w.ld];
            base_out[i] = w.base[i];
        }
        if (threadIdx.x == 0) {
            BatchRes r;
            r.opt = w.d[0];
            r.p1 = t.p1;
            r.p2 = t.p2;
            r.status = t.status == SX_EVICTED ? SX_NOT_ENDED : t.status;
            r.evicted = t.status == SX_EVICTED ? 1 : 0;
            a.res[id] = r;
        }
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device: every problem has the launch's one shape, problem k is the work
// counter's value, A, b and c are read in place through the caller's element strides, and the
// epilogue (wg_write_results) writes the caller's dense result arrays.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE) void k_batch_solve_dev(BatchDevArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    WG_SCRATCH(sc);
    double *const W = LDS ? s_dyn : a.ws + (size_t)blockIdx.x * (size_t)a.slice;
    const int n = a.n, m = a.m;
    const BatchWork w = wg_carve(W, n, m);
    const long long budget = a.budget > 0 ? a.budget : sx_batch_default_budget(n, m);
    // wg_by_col's rule, decided once: the strides are the launch's
    const bool by_col = (a.A_sc < 0 ? -a.A_sc : a.A_sc) <= (a.A_sr < 0 ? -a.A_sr : a.A_sr);
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                           a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t;
        WG_TWO_PHASE(t, w, src, by_col, a.max_pivots, budget, sc);
        wg_write_results(a, w, t, k, true);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_ragged: k_batch_solve_dev's strided source and on-device epilogue with
// k_batch_solve's per-problem carve.  a.n x a.m is the envelope that shapes every input and output
// array; problem k is the n_k[k] x m_k[k] leading block of its slot, and only that block is read.
// The dimensions are tested before anything is indexed with them; a problem that fails gets
// SX_BAD_SHAPE and cleared outputs.  The outputs keep the envelope's dense shapes: x +0.0 and base
// -1 behind the problem's own lengths, the objective row in envelope columns (structural entries at
// 1 + j, slack entries at 1 + n + i, artificial entries at 1 + n + m + i), +0.0 everywhere else.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE) void k_batch_solve_rag(BatchRagArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    WG_SCRATCH(sc);
    double *const W = LDS ? s_dyn : a.ws + (size_t)blockIdx.x * (size_t)a.slice;
    const int n = a.n, m = a.m, N1 = 1 + n + 2 * m;
    // wg_by_col's rule, decided once: the strides are the launch's
    const bool by_col = (a.A_sc < 0 ? -a.A_sc : a.A_sc) <= (a.A_sr < 0 ? -a.A_sr : a.A_sr);
    for (;;) {
        const unsigned turn = wg_next(a.counter, sc);
        if (turn >= (unsigned)a.count) return;
        // the problem and its dimensions are the same in every lane: kept in scalar registers
        const int k = __builtin_amdgcn_readfirstlane(a.order != nullptr ? a.order[turn] : (int)turn);
        if ((unsigned)k >= (unsigned)a.count) {  // not a problem of this call: skipped
            __syncthreads();                     // (sc.k is rewritten next)
            continue;
        }
        const int nk = __builtin_amdgcn_readfirstlane(a.n_k[k]), mk = __builtin_amdgcn_readfirstlane(a.m_k[k]);
        const bool good = nk >= 1 && mk >= 1 && nk <= n && mk <= m && sx_batch_lay(nk, mk).total <= a.set;
        // a problem that fails the test is carried through the epilogue as 0 x 0: nothing is carved
        // for it, nothing of it is read, and every output is cleared
        const int en = good ? nk : 0, em = good ? mk : 0, Ns = 1 + en + em;
        const BatchWork w = wg_carve(W, en, em);
        TwoPhase t{SX_BAD_SHAPE, false, 0, 0};
        if (good) {
            const long long budget = a.budget > 0 ? a.budget : sx_batch_default_budget(en, em);
            const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                               a.c + (long long)k * a.c_sb, a.c_sj};
            WG_TWO_PHASE(t, w, src, by_col, a.max_pivots, budget, sc);
        }
        const bool feasible = t.status == SX_FEASIBLE, evicted = t.status == SX_EVICTED;
        if (a.x != nullptr) {
            // k_batch_solve_dev's staging in the pivot-row copy, over the problem's own entries
            for (int j = threadIdx.x; j < en; j += SX_TILE) w.prow[j] = 0.0;
            __syncthreads();
            if (feasible)
                for (int i = threadIdx.x; i < em; i += SX_TILE) {
                    const unsigned bi = (unsigned)w.base[i];
                    if (bi < (unsigned)en) w.prow[bi] = w.T[(size_t)i * w.ld];
                }
            __syncthreads();
            double *x = a.x + (size_t)k * (size_t)n;
            for (int j = threadIdx.x; j < n; j += SX_TILE) x[j] = j < en ? w.prow[j] : 0.0;
        }
        if (a.base != nullptr) {
            int *base_out = a.base + (size_t)k * (size_t)m;
            for (int i = threadIdx.x; i < m; i += SX_TILE) base_out[i] = i < em ? w.base[i] : -1;
        }
        // the problem's own logical width, as k_batch_solve_dev reports it
        const int width = evicted || !good ? 0 : t.ph2 ? Ns : Ns + em;
        if (a.objrow != nullptr) {
            double *row = a.objrow + (size_t)k * (size_t)N1;
            for (int j = threadIdx.x; j < N1; j += SX_TILE) {
                // envelope column j -> the problem's logical column l, or -1 where it has none
                int l;
                if (j <= n)
                    l = j <= en ? j : -1;
                else if (j <= n + m)
                    l = j - n - 1 < em ? 1 + en + (j - n - 1) : -1;
                else
                    l = j - n - m - 1 < em ? Ns + (j - n - m - 1) : -1;
                row[j] = l >= 0 && l < width ? w.d[l] : 0.0;
            }
        }
        if (threadIdx.x == 0) {
            a.status[k] = evicted ? SX_NOT_ENDED : t.status;
            a.pivots[2 * (size_t)k] = t.p1;
            a.pivots[2 * (size_t)k + 1] = t.p2;
            a.opt[k] = feasible ? w.d[0] : __builtin_nan("");
            if (a.row_width != nullptr) a.row_width[k] = width;
            if (evicted) atomicAdd(a.evicted, 1);
        }
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_state: k_batch_solve_dev with a saved state per problem (sx_common.hpp
// BatchState: the stored columns of T dense at stride 1 + n + m, d at full width, the basis, the phase
// and both pivot counts).  Without a.in a problem is built and solved as there; with it the working
// set is loaded from the state instead and the same loop is re-entered -- phase 1 behind its saved
// pivots, then phase 2 from 0 with the call's costs; or phase 2 behind its saved pivots, or, with
// a.recost, from 0 on the row of the call's costs made canonical for the saved basis.  No outcome
// has a case of its own: selection writes nothing, so a state whose phase had ended ends again
// without a pivot.  The state is tested first (WG_STATE_TEST); a problem that fails gets SX_BAD_STATE
// and cleared outputs.  The end is WG_KEPT_END's.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE) void k_batch_solve_st(BatchStArgs a) {
    WG_KEPT_HEAD(a, sc);
    WG_KEPT_CARVE(a, );
    const bool resume = a.in.T != nullptr;
    const int cells = m * Ns;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        // a resume reads only c
        const SxSource src{resume ? nullptr : a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc,
                           resume ? nullptr : a.b + (long long)k * a.b_sb, a.b_si, a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool good = true;
        if (!resume) {
            wg_build(w, src, by_col);
            wg_update_objective(w, N1);
        } else {
            WG_STATE_TEST(good, a.in, k, ph == 1 || ph == 2, n, m, m, WG_BASE_ROW(w), );
            if (good) {
                // consecutive lanes walk the dense rows; the working set's stride is the odd ld
                WG_LOAD_STATE(a.in);
                __syncthreads();
                t.p1 = q1;
                t.p2 = q2;
                t.ph2 = ph == 2;
            }
        }
        if (good) {
            if (!t.ph2) {
                WG_PHASE1(t, w, N1, a.max_pivots, budget, t.p1, sc);
                if (t.ph2) {
                    wg_phase2_costs(w, src);
                    wg_update_objective(w, Ns);
                    t.p2 = 0;
                }
            } else if (a.recost) {
                // the warm start: the call's costs on the saved tableau, the objective from +0.0
                if (threadIdx.x == 0) w.d[0] = 0.0;
                wg_phase2_costs(w, src);
                wg_update_objective(w, Ns);
                t.p2 = 0;
            }
            if (t.ph2) WG_PHASE2(t, w, Ns, a.max_pivots, budget, t.p2, sc);
        }
        WG_KEPT_END(t, good, false);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_rhs: k_batch_solve_st's resume for a state that may stand inside the dual
// loop (phase 3: phase 2's tableau, primal infeasible), and with a.rerhs the re-solve of a kept state
// for the call's right-hand side b'.  wg_build starts from [D b | D A | D] (D = diag(+-1), its negation
// of a row, applied to the slack entry too) and every pivot is a row operation, so a kept tableau is
// M [D b | D A | D]: its slack block is S = M D, the RHS column of the same basis on b' is S b' and its
// objective y b' with y the slack entries of d; d itself does not depend on b.  While d is still dual
// feasible that is the warm start:
// the new column and objective in wg_update_objective's order, the dual loop (wg_dual) from pivot 0
// until the column is primal feasible, then phase 2 at the same count, which makes no pivot unless
// rounding left an entry of d below -eps.  A phase-1 state, or a row that is not dual feasible
// (WG_DUAL_LOST: a state that ended UNBOUNDED or was capped in phase 2), is a cold start from A, b', c
// (WG_COLD_START).  Without a.rerhs A and b are not read; phase-1 and phase-2 states are
// k_batch_solve_st's resume and a phase-3 state re-enters the dual loop behind its saved pivots.  The
// state's tests are k_batch_solve_st's with phase 3 (the basis range is phase 2's); the loops and the
// end are WG_KEPT_TAIL's and WG_KEPT_END's.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_rhs(BatchRhsArgs a) {
    WG_KEPT_HEAD(a, sc);
    WG_KEPT_CARVE(a, );
    const bool rerhs = a.rerhs != 0;
    const int cells = m * Ns;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        // a plain resume reads only c
        const SxSource src{rerhs ? a.A + (long long)k * a.A_sb : nullptr, a.A_sr, a.A_sc,
                           rerhs ? a.b + (long long)k * a.b_sb : nullptr, a.b_si, a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        WG_STATE_TEST(bool good, a.in, k, ph >= 1 && ph <= 3, n, m, m, WG_BASE_ROW(w), );
        if (good) {
            bool cold = rerhs && ph == 1;
            if (!cold) {
                // consecutive lanes walk the dense rows; the working set's stride is the odd ld
                WG_LOAD_STATE(a.in);
                // the new right-hand side, staged in the pivot-row copy (1 + n + m >= m doubles)
                if (rerhs)
                    for (int i = threadIdx.x; i < m; i += SX_TILE) w.prow[i] = src.b[(long long)i * src.b_si];
                __syncthreads();
                t.p1 = q1;
                t.p2 = q2;
                t.ph2 = ph >= 2;
                dual = ph == 3;
                if (rerhs) WG_DUAL_LOST(cold, w, Ns);
            }
            if (cold) {
                WG_COLD_START(t, dual, wg_build(w, src, by_col));
            } else if (rerhs) {
                // T[i][0] = S[i][.] b' and, as row m, d[0] = y b'
                for (int i = threadIdx.x; i <= m; i += SX_TILE) {
                    WG_SLACK_DOT(s, i);
                    (i < m ? w.T[(size_t)i * w.ld] : w.d[0]) = s;
                }
                __syncthreads();
                t.p2 = 0;
                dual = true;
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_rows: a kept state of shape (n, m0) grown by q = a.added constraint rows
// to the call's shape (n, m = m0 + q) and re-solved: k_batch_solve_rhs with another front.  The grown
// system is [D' b' | D' A' | D'] with D' = diag(D, I), and a new row minus a combination of old rows is
// a row operation on it, so the grown tableau is again M' [D' b' | D' A' | D'] with the slack block
// S' = [[S, 0], [-f^T S, I]]: k_batch_solve_rhs's identities hold on it.
// The front is the row-growing one, which k_batch_solve_branch and k_batch_solve_cut share: the
// state's tests against the in-state's shape with the new rows' slacks basic (WG_STATE_TEST with
// WG_GROWN_ROW), the load (WG_LOAD_GROWN), and per new row the reduction against the kept basis
// (WG_REDUCE_ROW).  A phase-1 state, or a row d that is not dual feasible, is a cold start from A, b, c
// (WG_COLD_START).  This kernel's own: a new row is read, row r of A and b through their strides, with
// its unit slack.  The new rows do not depend on each other, d is unchanged, pivots[0] is kept and
// pivots[1] = 0; then the dual loop from 0 and phase 2 at the same count (WG_KEPT_TAIL).  Only rows
// m0 .. m of A and b are read unless the problem is cold.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_rows(BatchRowsArgs a) {
    WG_KEPT_HEAD(a, sc);
    const int q = a.added, m0 = m - q, Ns0 = Ns - q, N10 = Ns0 + m0;  // the in-state's shape
    WG_KEPT_CARVE(a, );
    const int cells = m * Ns, cells0 = m0 * Ns0;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                           a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        WG_STATE_TEST(bool good, a.in, k, ph >= 1 && ph <= 3, n, m0, m, WG_GROWN_ROW(w, m0), );
        if (good) {
            bool cold = ph == 1;
            if (!cold) {
                WG_LOAD_GROWN(a.in, k, q);
                WG_DUAL_LOST(cold, w, Ns);  // at the grown width
            }
            if (cold) {
                WG_COLD_START(t, dual, wg_build(w, src, by_col));
            } else {
                for (int r = m0; r < m; ++r) {
                    const double *Ar = src.A + (long long)r * src.A_sr;
                    WG_REDUCE_ROW(r, bi < n ? Ar[(long long)bi * src.A_sc] : 0.0,
                                  j == 0   ? src.b[(long long)r * src.b_si]
                                  : j <= n ? Ar[(long long)(j - 1) * src.A_sc]
                                           : (j - 1 - n == r ? 1.0 : 0.0));
                }
                t.p1 = q1;
                t.p2 = 0;
                t.ph2 = dual = true;
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_cols: a kept state of shape (n0, m) grown by p = a.added structural columns
// to the call's shape (n = n0 + p, m) and re-solved: k_batch_solve_rows with another front.  A kept
// tableau is M [D b | D A | D] with the slack block S = M D (k_batch_solve_rhs), so the stored form of a
// new structural column a is M D a = S a and its reduced cost y a - c_new, y the slack entries of d: the
// re-rhs pass's two sums (WG_SLACK_DOT), once per new column.  S does not change, so the right-hand-side entry's
// identities hold on the grown state.
// Load: the dense in-state is walked at its stride 1 + n0 + m into the grown working set (odd ld of the
// grown shape); the structural block grows in the middle, so stored column j < 1 + n0 stays and the
// slack column 1 + n0 + k moves to 1 + n + k, in T and in d, d ends in +0.0 from 1 + n + m on, and a
// basic slack's index moves up by p.  New column t: column n0 + t of A is staged through its strides
// in the pivot-row copy, then consecutive lanes take consecutive rows (row m is d; the odd ld keeps the
// gather of S[i][k] conflict-free) and sum in wg_update_objective's order; c is subtracted from row
// m's sum in one rounded operation.  d[0], the RHS column and the old columns are unchanged, pivots[0]
// is kept and pivots[1] = 0.  The old basis stays primal feasible, so a phase-2 state is always warm:
// phase 2 from 0 at the grown width, whatever its old status was.  A phase-3 state re-enters the dual
// loop (wg_dual) from 0 while the grown d is still dual feasible, then phase 2 at the same count; a
// phase-1 state, or a phase-3 state whose grown row is not dual feasible, is a cold start from A, b, c
// (WG_COLD_START).  The state's tests are k_batch_solve_rhs's against the in-state's shape.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_cols(BatchColsArgs a) {
    WG_KEPT_HEAD(a, sc);
    const int p = a.added, n0 = n - p, Ns0 = Ns - p, N10 = Ns0 + m;  // the in-state's shape
    WG_KEPT_CARVE(a, );
    const int cells = m * Ns, cells0 = m * Ns0;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                           a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        // the in-state's own range: what is valid only for the grown shape is refused
        WG_STATE_TEST(
            bool good, a.in, k, ph >= 1 && ph <= 3, n0, m, m,
            {
                const int bi = base_in[i];
                w.base[i] = bi >= n0 ? bi + p : bi;  // a slack moves up with its column
                bad |= (unsigned)bi >= lim;
            }, );
        if (good) {
            bool cold = ph == 1;
            if (!cold) {
                // consecutive lanes walk the dense rows of the in-state; the working set's stride is
                // the grown shape's odd ld, and the slack block lands p columns further on
                const double *T_in = a.in.T + (size_t)k * (size_t)cells0;
                for (int x = threadIdx.x; x < cells0; x += SX_TILE) {
                    const int i = x / Ns0, j = x - i * Ns0;
                    w.T[(size_t)i * w.ld + (j <= n0 ? j : j + p)] = T_in[x];
                }
                const double *d_in = a.in.d + (size_t)k * (size_t)N10;
                for (int j = threadIdx.x; j < N1; j += SX_TILE)
                    w.d[j] = j <= n0 ? d_in[j] : j > n && j < Ns ? d_in[j - p] : 0.0;
                for (int c = 0; c < p; ++c) {
                    // the new column, staged in the pivot-row copy (1 + n + m >= m doubles)
                    const double *Ac = src.A + (long long)(n0 + c) * src.A_sc;
                    for (int i = threadIdx.x; i < m; i += SX_TILE) w.prow[i] = Ac[(long long)i * src.A_sr];
                    __syncthreads();  // (the first one also completes the load)
                    // T[i][1 + n0 + c] = S[i][.] a and, as row m, d[1 + n0 + c] = y a - c_new
                    for (int i = threadIdx.x; i <= m; i += SX_TILE) {
                        WG_SLACK_DOT(s, i);
                        if (i < m)
                            w.T[(size_t)i * w.ld + 1 + n0 + c] = s;
                        else
                            w.d[1 + n0 + c] = s - src.c[(long long)(n0 + c) * src.c_sj];
                    }
                    __syncthreads();  // prow is rewritten for the next column; T and d are complete behind the last
                }
                if (ph == 3) WG_DUAL_LOST(cold, w, Ns);  // at the grown width
            }
            if (cold) {
                WG_COLD_START(t, dual, wg_build(w, src, by_col));
            } else {
                t.p1 = q1;
                t.p2 = 0;
                t.ph2 = true;
                dual = ph == 3;
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// The tableau of the working set wc with tableau row di (none: di >= wc.m) and stored column dj deleted,
// moved into wn, the carve of the shape that is left, in the same buffer: T, then d on [0, Ns), then the
// basis, whose entries above the deleted variable v go down by one.  Everything moves to lower
// addresses -- every offset of sx_batch_lay grows with the shape, T lies in front of d, d in front of
// the basis, and the cells are walked in ascending order of both addresses -- so a 512-cell chunk is
// read into registers, then a barrier, then written: no cell is overwritten before it is read, and what
// a chunk writes lies below everything a later chunk reads.  Ends behind a barrier.
__device__ __forceinline__ void wg_shrink(const BatchWork &wc, const BatchWork &wn, int di, int dj, int v) {
    const int Nsn = 1 + wn.n + wn.m, cells = wn.m * Nsn;
    for (int x0 = 0; x0 < cells; x0 += SX_TILE) {
        const int x = x0 + (int)threadIdx.x, i = x / Nsn, j = x - i * Nsn;
        double val = 0.0;
        if (x < cells) val = wc.T[(size_t)(i + (i >= di)) * wc.ld + (j + (j >= dj))];
        __syncthreads();
        if (x < cells) wn.T[(size_t)i * wn.ld + j] = val;
    }
    for (int j0 = 0; j0 < Nsn; j0 += SX_TILE) {
        const int j = j0 + (int)threadIdx.x;
        double val = 0.0;
        if (j < Nsn) val = wc.d[j + (j >= dj)];
        __syncthreads();
        if (j < Nsn) wn.d[j] = val;
    }
    for (int i0 = 0; i0 < wn.m; i0 += SX_TILE) {
        const int i = i0 + (int)threadIdx.x;
        int bi = 0;
        if (i < wn.m) bi = wc.base[i + (i >= di)];
        __syncthreads();
        if (i < wn.m) wn.base[i] = bi - (bi > v);
    }
    __syncthreads();
}

// the tableau row in which variable v is basic, or -1, through the argmin's result slot; uniform over
// the workgroup.  A basis names a variable once; of a state that names it twice one of the rows is
// taken.  Ends behind a barrier: the slot is free again.
__device__ __forceinline__ int wg_basic_row(const BatchWork &w, int v, const WgScratch &sc) {
    if (threadIdx.x == 0) sc.ri = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < w.m; i += SX_TILE)
        if (w.base[i] == v) sc.ri = i;
    __syncthreads();
    const int r = sc.ri;
    __syncthreads();
    return r;
}

// The drops of one problem (k_batch_solve_drop): the q variables ix[0] < .. < ix[q - 1] -- the slacks
// of constraint rows (kind 0) or structural columns (kind 1) -- leave the tableau loaded at W in the
// in-state's shape (n, m), last index first, each at the shape the earlier ones left: the tableau is
// re-carved after every drop (wg_shrink), so the selections see the current shape's positions and
// lengths and the last carve is the reduced shape's.
//   a row whose slack is basic, a column that is nonbasic: deleted, no arithmetic;
//   a row whose slack is nonbasic: the slack is forced in.  It is about to leave the problem, so it may
//   move in either direction: with an entry >= eps in its column the leaving row is wg_solve's ratio
//   argmin; else with an entry <= -eps the same argmin on the negated column (the pivot element is then
//   negative, the other right-hand sides stay non-negative and the row itself is the one deleted);
//   a basic column: forced out by a dual pivot on its row i, the entering variable the eps-argmin of
//   d[1 + j] / (s T[i][1 + j]) over the other columns with s T[i][1 + j] >= eps, s the sign that leaves
//   row i primal feasible.
// Returns the number of forced pivots (WG_PIVOT, the loops' pivot), or -1 when a forced selection found
// no candidate: the problem is then solved cold.  Uniform over the workgroup; ends behind a barrier.
__device__ __forceinline__ int wg_drop(double *W, int n, int m, int kind, int q, const int *ix, const WgScratch &sc) {
    int forced = 0;
    for (int t = q - 1; t >= 0; --t) {
        const BatchWork w = wg_carve(W, n, m);
        const int ld = w.ld, Ns = 1 + n + m, art0 = Ns;
        const int v = kind == 0 ? n + ix[t] : ix[t];  // the variable that leaves the problem
        int r = wg_basic_row(w, v, sc);
        if ((kind == 0) == (r < 0)) {
            WG_ROW_LANES();
            int e;
            double rv;
            if (kind == 0) {
                int pos = 0, neg = 0;
                for (int i = threadIdx.x; i < m; i += SX_TILE) {
                    const double a = w.T[(size_t)i * ld + 1 + v];
                    w.colE[i] = a;
                    pos |= a >= SX_EPS;
                    neg |= -a >= SX_EPS;
                }
                pos = __syncthreads_or(pos);
                neg = __syncthreads_or(neg);
                if (!pos && !neg) return -1;
                const bool down = !pos;
                wg_argmin(
                    m,
                    [&](int i) {
                        const double a = down ? -w.colE[i] : w.colE[i], b = w.T[(size_t)i * ld];
                        return cmp_eps(a, 0.0) > 0 ? b / a : DBL_MAX;
                    },
                    w.parts, sc, rv, r);
                if (r < 0 || r >= m) return -1;
                e = v;
            } else {
                const double *lrow = w.T + (size_t)r * ld;
                const bool minus = cmp_eps(lrow[0], 0.0) < 0;
                int any = 0;
                for (int j = threadIdx.x; j < Ns - 1; j += SX_TILE)
                    any |= j != v && (minus ? -lrow[1 + j] : lrow[1 + j]) >= SX_EPS;
                if (!__syncthreads_or(any)) return -1;
                wg_argmin(
                    Ns - 1,
                    [&](int idx) {
                        const double a = minus ? -lrow[1 + idx] : lrow[1 + idx];
                        return idx != v && cmp_eps(a, 0.0) > 0 ? w.d[1 + idx] / a : DBL_MAX;
                    },
                    w.parts, sc, rv, e);
                if (e < 0 || e >= Ns - 1) return -1;
                for (int i = threadIdx.x; i < m; i += SX_TILE) w.colE[i] = w.T[(size_t)i * ld + 1 + e];
            }
            const int ce = 1 + e;
            const double d_e = w.d[ce];
            WG_PIVOT(Ns, r, e, ce, d_e);
            ++forced;
        }
        if (kind == 0) {
            wg_shrink(w, wg_carve(W, n, m - 1), r, 1 + v, v);
            --m;
        } else {
            wg_shrink(w, wg_carve(W, n - 1, m), m, 1 + v, v);
            --n;
        }
    }
    return forced;
}

// simplex_solve_batch_device_drop: a kept state of shape (n, m + q) (a.kind 0: q = a.dropped constraint
// rows leave) or (n + q, m) (a.kind 1: structural columns) reduced to the call's shape (n, m) and
// re-solved: k_batch_solve_cols with another front.  a.kind is a uniform branch, not a template
// parameter.  The working set -- dynamic LDS or slice -- is the in-state's shape's, because the forced
// pivots run there; problem k's own indices are a.idx[k][.], strictly ascending and inside the
// in-state's shape, else the problem gets SX_BAD_STATE as a state that fails its range test does.
// The in-state is loaded at its own shape and the drops are applied by wg_drop.  Warm or cold: a
// phase-1 state is cold; a phase-3 state with row drops is warm only if every dropped slack is basic (a
// forced primal pivot needs a primal feasible column); column drops one of which is basic are warm only
// while the loaded d is dual feasible (wg_solve's entering selection over d[1 .. Ns_in), once, before
// the first drop), because the forced dual pivot keeps that; a forced selection without a candidate
// makes the problem cold.  A cold problem is built from A, b, c of the reduced problem
// (WG_COLD_START).  The forced pivots belong to the load: pivots[0] is kept, pivots[1] starts at
// their number f, neither the cap nor the budget counts them, and the loops behind start at f: the dual
// loop (wg_dual) for a phase-3 state and behind a forced dual pivot, then phase 2 at the same count;
// phase 2 alone otherwise.  A basic slack's column is a unit column and a nonbasic column stands in no
// identity, so the reduced tableau is M' [D' b' | D' A' | D'] again and k_batch_solve_rhs's identities
// hold on it.  The state's tests are k_batch_solve_rhs's against the in-state's shape.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_drop(BatchDropArgs a) {
    WG_KEPT_HEAD(a, sc);
    const int kind = a.kind, q = a.dropped;
    const int n0 = kind == 0 ? n : n + q, m0 = kind == 0 ? m + q : m;  // the in-state's shape
    const int Ns0 = 1 + n0 + m0, N10 = Ns0 + m0;
    WG_KEPT_CARVE(a, const BatchWork w0 = wg_carve(W, n0, m0));
    const int cells = m * Ns, cells0 = m0 * Ns0;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                           a.c + (long long)k * a.c_sb, a.c_sj};
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        const int *ix = a.idx + (size_t)k * (size_t)q;
        // the in-state's own range, and the list: strictly ascending inside that shape
        WG_STATE_TEST(
            bool good, a.in, k, ph >= 1 && ph <= 3, n0, m0, m0, WG_BASE_ROW(w0),
            for (int j = threadIdx.x; j < q; j += SX_TILE) {
                const int v = ix[j];
                bad |= (unsigned)v >= (unsigned)(kind == 0 ? m0 : n0) || (j > 0 && ix[j - 1] >= v);
            });
        if (good) {
            bool cold = ph == 1;
            int forced = 0;
            if (!cold) {
                // the in-state at its own shape
                wg_load_T(w0, a.in.T + (size_t)k * (size_t)cells0, Ns0, cells0);
                const double *d_in = a.in.d + (size_t)k * (size_t)N10;
                for (int j = threadIdx.x; j < N10; j += SX_TILE) w0.d[j] = d_in[j];
                __syncthreads();
                if (ph == 3 || kind == 1) {
                    int basic = 0;  // dropped variables that stand in the basis
                    for (int j = 0; j < q; ++j) basic += wg_basic_row(w0, kind == 0 ? n0 + ix[j] : ix[j], sc) >= 0;
                    if (kind == 0) {
                        cold = basic != q;
                    } else if (basic > 0) {
                        WG_DUAL_LOST(cold, w0, Ns0);  // at the in-state's width, before the first drop
                    }
                }
                if (!cold) {
                    forced = wg_drop(W, n0, m0, kind, q, ix, sc);
                    cold = forced < 0;
                }
            }
            if (cold) {
                WG_COLD_START(t, dual, wg_build(w, src, by_col));
            } else {
                t.p1 = q1;
                t.p2 = forced;
                t.ph2 = true;
                dual = ph == 3 || (kind == 1 && forced > 0);
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// wg_build of a child of k_batch_solve_branch: orc_build_phase1 of the composite problem whose rows
// [0, mA) are the root's at src, read through its strides, and whose row mA + t is the bound row
// cf[t] x_var[t] <= rh[t]: cf[t] at column var[t], +0.0 elsewhere.  The same copies, the same negation
// of a row with compare(b_i) < 0 across all its entries, and the same walk of A's faster-varying
// dimension as wg_build, which stays as it is under the other kernels.  Ends behind a barrier.
__device__ __forceinline__ void wg_build_branch(const BatchWork &w, const SxSource &src, bool by_col, int mA,
                                                const int *var, const double *cf, const double *rh) {
    const int n = w.n, m = w.m, ld = w.ld;
    const auto rhs_of = [&](int i) { return i < mA ? src.b[(long long)i * src.b_si] : rh[i - mA]; };
    const auto structural = [&](int i, int j) {
        const double v = i < mA               ? src.A[(long long)i * src.A_sr + (long long)j * src.A_sc]
                         : j == var[i - mA] ? cf[i - mA]
                                            : 0.0;
        w.T[(size_t)i * ld + 1 + j] = cmp_eps(rhs_of(i), 0.0) < 0 ? -v : v;
    };
    if (by_col) {
        for (int x = threadIdx.x; x < n * m; x += SX_TILE) structural(x / n, x % n);
    } else {
        for (int x = threadIdx.x; x < n * m; x += SX_TILE) structural(x % m, x / m);
    }
    for (int x = threadIdx.x; x < m * (m + 1); x += SX_TILE) {
        const int i = x / (m + 1), t = x - i * (m + 1);
        const double b = rhs_of(i);
        const double v = t == 0 ? b : (t - 1 == i ? 1.0 : 0.0);
        w.T[(size_t)i * ld + (t == 0 ? 0 : n + t)] = cmp_eps(b, 0.0) < 0 ? -v : v;
    }
    for (int j = threadIdx.x; j < 1 + n + 2 * m; j += SX_TILE) w.d[j] = j <= n + m ? 0.0 : 1.0;
    for (int i = threadIdx.x; i < m; i += SX_TILE) w.base[i] = n + m + i;
    __syncthreads();
}

// simplex_solve_batch_device_branch: k_batch_solve_rows with added = 1 for the children of a branch.
// Child k of the call's shape (n, m) continues the kept state of problem pk = a.parent[k], shape
// (n, m - 1), on the problem rk = a.root[k] of the source, which holds a.roots problems of mA = m - q
// rows (q = a.depth); behind the root's rows come the child's q bound rows cf[t] x_var[t] <= rh[t], of
// which the first q - 1 are what the parent was solved with and the last one is new.  No dense row
// exists: the new row's raw entries are rh[q - 1] | cf[q - 1] at column var[q - 1], +0.0 elsewhere | the
// unit slack, and its multipliers are cf[q - 1] where base[i] == var[q - 1] and +0.0 elsewhere; these
// go to the shared chain (WG_REDUCE_ROW), so every bit is k_batch_solve_rows's on the explicit grown
// problem.  The cold start builds the composite problem (wg_build_branch).
// The in-state is indexed with pk and the source with rk; results and out-state are written at k.  pk,
// rk and the q variables are tested before anything is indexed with them, so the phase and the pivot
// counts are read here, under that test, and not by WG_STATE_TEST, which reads them unconditionally;
// the basis test is its second half (WG_STATE_BASIS).  A child that fails gets SX_BAD_STATE and
// cleared outputs.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_branch(BatchBranchArgs a) {
    WG_KEPT_HEAD(a, sc);
    const int q = a.depth, mA = m - q, m0 = m - 1, Ns0 = Ns - 1, N10 = Ns0 + m0;  // the in-state's shape
    WG_KEPT_CARVE(a, );
    const int cells = m * Ns, cells0 = m0 * Ns0;  // (a working set holds them, so they fit an int)
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const int pk = a.parent[k], rk = a.root[k];
        const int *var = a.var + (size_t)k * (size_t)q;
        const double *cf = a.coef + (size_t)k * (size_t)q, *rh = a.rhs + (size_t)k * (size_t)q;
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        // the child's own indices, before the in-state or the source is indexed with them
        int off = 0;
        for (int j = threadIdx.x; j < q; j += SX_TILE) off |= (unsigned)var[j] >= (unsigned)n;
        bool good = !__syncthreads_or(off) && (unsigned)pk < (unsigned)a.parents && (unsigned)rk < (unsigned)a.roots;
        // the in-state's own tests, against its shape, at pk: only a pk in range is read
        int ph = 0;
        long long q1 = 0, q2 = 0;
        if (good) {
            ph = a.in.phase[pk];
            q1 = a.in.pivots[2 * (size_t)pk];
            q2 = a.in.pivots[2 * (size_t)pk + 1];
            good = ph >= 1 && ph <= 3 && q1 >= 0 && q2 >= 0;
        }
        WG_STATE_BASIS(a.in, pk, n, m0, m, WG_GROWN_ROW(w, m0), );
        if (good) {
            const SxSource src{a.A + (long long)rk * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)rk * a.b_sb, a.b_si,
                               a.c + (long long)rk * a.c_sb, a.c_sj};
            bool cold = ph == 1;
            if (!cold) {
                WG_LOAD_GROWN(a.in, pk, 1);
                WG_DUAL_LOST(cold, w, Ns);  // at the child's width
            }
            if (cold) {
                WG_COLD_START(t, dual, wg_build_branch(w, src, by_col, mA, var, cf, rh));
            } else {
                const int v = var[q - 1];
                const double cv = cf[q - 1], rv = rh[q - 1];
                WG_REDUCE_ROW(m0, bi == v ? cv : 0.0,
                              j == 0 ? rv : j <= n ? (j - 1 == v ? cv : 0.0) : (j - 1 - n == m0 ? 1.0 : 0.0));
                t.p1 = q1;
                t.p2 = 0;
                t.ph2 = dual = true;
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// simplex_solve_batch_device_cut: k_batch_solve_rows whose q = a.cuts new rows are not read but
// produced: Gomory mixed-integer cuts of the kept optimum, written in the caller's variables into
// a.cut_A and a.cut_b (the wrapper points them at rows m0 .. m of the caller's grown A and b), then
// reduced and re-solved exactly as that kernel does with rows it reads.  The front
// never re-reads from global memory what the launch wrote: an emitted row is produced in the working
// set -- straight in T[m0 + t][0 .. n], where the raw row of k_batch_solve_rows's chain stands --, is
// stored from there with plain vector stores, and is consumed from there.  Only rows [0, m0) of A and b
// are read.
// Usable: a phase-2 state whose row is dual feasible at the grown width, a kept optimum.  Cut t of a
// usable problem: the source row is the eps-argmin (wg_argmin) of -min(f0, 1 - f0) over the rows whose
// basic variable is an integer structural, whose right-hand side has the fractional part f0 in
// [away, 1 - away] and which no earlier cut of the call took (marks in colE), or the caller's row[k][t]
// if it is such a row.  Its coefficients g over the stored columns [0, n + m0) go to the pivot-row
// copy, which first holds the basic columns' marks: a lane reads the mark of the element it then
// writes.  Then consecutive lanes take consecutive structural columns j (lane n: the right-hand side),
// start at -g_j (-f0) and add g_{n+i} A[i][j] (b[i]) for i = 0 .. m0 - 1 in that order by fma, the
// accumulator in a register and g_{n+i} an LDS broadcast.  That is one pass over A per cut: q is the
// call's, not the compiler's, so the q accumulators of a single pass have no registers to live in.
// Every other cut is the null row, +0.0 throughout; a cold problem's cuts are all null, so its
// composite build is wg_build_branch's with +0.0 coefficients and right-hand sides (staged in colE).
// The state's tests, the load and the reduction of each new row are the row-growing front's
// (k_batch_solve_rows), the multipliers taken from the raw row where it stands before the chain
// overwrites it; then the shared tail and the shared end.
template <bool LDS>
__global__ __launch_bounds__(SX_TILE, 4) void k_batch_solve_cut(BatchCutArgs a) {
    WG_KEPT_HEAD(a, sc);
    const int q = a.cuts, m0 = m - q, Ns0 = Ns - q, N10 = Ns0 + m0;  // the in-state's shape
    WG_KEPT_CARVE(a, );
    const int cells = m * Ns, cells0 = m0 * Ns0;  // (a working set holds them, so they fit an int)
    const double away = a.away;
    for (;;) {
        const unsigned k = wg_next(a.counter, sc);
        if (k >= (unsigned)a.count) return;
        const SxSource src{a.A + (long long)k * a.A_sb, a.A_sr, a.A_sc, a.b + (long long)k * a.b_sb, a.b_si,
                           a.c + (long long)k * a.c_sb, a.c_sj};
        const unsigned char *isint = a.integer + (long long)k * a.integer_sb;
        double *const cA = a.cut_A + (long long)k * a.cut_A_sb, *const cb = a.cut_b + (long long)k * a.cut_b_sb;
        int *const crow = a.cut_row + (size_t)k * (size_t)q;
        TwoPhase t{SX_BAD_STATE, false, 0, 0};
        bool dual = false;  // the problem stands inside the dual loop
        WG_STATE_TEST(bool good, a.in, k, ph >= 1 && ph <= 3, n, m0, m, WG_GROWN_ROW(w, m0), );
        bool cold = !good || ph == 1;
        if (!cold) {
            WG_LOAD_GROWN(a.in, k, q);
            WG_DUAL_LOST(cold, w, Ns);  // at the grown width
        }
        if (cold) {
            // no cut: null rows, and nothing of the source row in cut_row
            for (int x = threadIdx.x; x < q * (n + 1); x += SX_TILE) {
                const int tt = x / (n + 1), j = x - tt * (n + 1);
                if (j < n)
                    cA[(long long)tt * a.cut_A_sr + (long long)j * a.cut_A_sc] = 0.0;
                else
                    cb[(long long)tt * a.cut_b_si] = 0.0;
            }
            for (int tt = threadIdx.x; tt < q; tt += SX_TILE) crow[tt] = -1;
        }
        if (good) {
            if (cold) {
                // the composite build of the m0 rows read and q rows of +0.0
                for (int tt = threadIdx.x; tt < q; tt += SX_TILE) w.colE[tt] = 0.0;
                __syncthreads();
                WG_COLD_START(
                    t, dual,
                    wg_build_branch(w, src, by_col, m0, reinterpret_cast<const int *>(w.colE), w.colE, w.colE));
            } else {
                const bool usable = ph == 2;
                for (int i = threadIdx.x; i < m0; i += SX_TILE) w.colE[i] = 0.0;  // no row is taken yet
                __syncthreads();
                for (int tt = 0; tt < q; ++tt) {
                    double *row = w.T + (size_t)(m0 + tt) * w.ld;
                    // the key of row i; DBL_MAX: not eligible
                    const auto key = [&](int i) {
                        const int v = w.base[i];
                        if (v >= n || w.colE[i] != 0.0 || isint[(long long)v * a.integer_sj] == 0) return DBL_MAX;
                        const double t0 = w.T[(size_t)i * w.ld], f0 = t0 - floor(t0), f1 = 1.0 - f0;
                        return f0 >= away && f1 >= away ? -fmin(f0, f1) : DBL_MAX;
                    };
                    int r = -1;
                    if (usable) {
                        if (a.row == nullptr) {
                            double kv;
                            wg_argmin(m0, key, w.parts, sc, kv, r);
                            if (kv == DBL_MAX || r < 0 || r >= m0) r = -1;
                        } else {
                            r = a.row[(size_t)k * (size_t)q + tt];
                            if (r < 0 || r >= m0 || key(r) == DBL_MAX) r = -1;
                        }
                    }
                    if (r >= 0) {
                        const double *rowr = w.T + (size_t)r * w.ld;
                        const double t0 = rowr[0], f0 = t0 - floor(t0), rho = f0 / (1.0 - f0);
                        // the basic columns' marks, then g over them
                        for (int jj = threadIdx.x; jj < n + m0; jj += SX_TILE) w.prow[jj] = 0.0;
                        __syncthreads();
                        for (int i = threadIdx.x; i < m0; i += SX_TILE) w.prow[w.base[i]] = 1.0;
                        __syncthreads();
                        for (int jj = threadIdx.x; jj < n + m0; jj += SX_TILE) {
                            const double al = rowr[1 + jj];
                            double g = 0.0;
                            if (w.prow[jj] == 0.0 && cmp_eps(al, 0.0) != 0) {
                                if (jj < n && isint[(long long)jj * a.integer_sj] != 0) {
                                    const double fj = al - floor(al);
                                    g = fj <= f0 ? fj : rho * (1.0 - fj);
                                } else {
                                    g = al > 0.0 ? al : rho * -al;
                                }
                            }
                            w.prow[jj] = g;
                        }
                        __syncthreads();
                        // the caller's variables: lane j < n column j of A, lane n the right-hand side
                        for (int j = threadIdx.x; j <= n; j += SX_TILE) {
                            const double *col = j < n ? src.A + (long long)j * src.A_sc : src.b;
                            const long long step = j < n ? src.A_sr : src.b_si;
                            double acc = j < n ? -w.prow[j] : -f0;
                            for (int i = 0; i < m0; ++i) acc = fma(w.prow[n + i], col[(long long)i * step], acc);
                            if (j < n) {
                                row[1 + j] = acc;
                                cA[(long long)tt * a.cut_A_sr + (long long)j * a.cut_A_sc] = acc;
                            } else {
                                row[0] = acc;
                                cb[(long long)tt * a.cut_b_si] = acc;
                            }
                        }
                    } else {
                        for (int j = threadIdx.x; j <= n; j += SX_TILE) {
                            row[j] = 0.0;
                            if (j < n)
                                cA[(long long)tt * a.cut_A_sr + (long long)j * a.cut_A_sc] = 0.0;
                            else
                                cb[(long long)tt * a.cut_b_si] = 0.0;
                        }
                    }
                    for (int i = threadIdx.x; i < m; i += SX_TILE) row[1 + n + i] = i == m0 + tt ? 1.0 : 0.0;
                    if (threadIdx.x == 0) {
                        crow[tt] = r;
                        if (r >= 0) w.colE[r] = 1.0;  // taken
                    }
                    __syncthreads();
                }
                // the raw row read from where it stands: the multipliers before the chain overwrites it
                for (int r = m0; r < m; ++r) WG_REDUCE_ROW(r, bi < n ? row[1 + bi] : 0.0, row[j]);
                t.p1 = q1;
                t.p2 = 0;
                t.ph2 = dual = true;
            }
            WG_KEPT_TAIL(t, dual);
        }
        WG_KEPT_END(t, good, dual);
        __syncthreads();  // the next problem overwrites the working set and sc.k
    }
}

// One entry's kernel pair: the dynamic-LDS attribute is set once per kernel.
template <class Args, void (*KL)(Args), void (*KW)(Args)>
struct Entry {
    static int resident(bool lds, size_t lds_bytes) {
        static bool attr_set = false;
        if (!attr_set) {
            SX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       SX_BATCH_LDS_BYTES));
            attr_set = true;
        }
        int device = 0, cus = 0, per_cu = 0;
        SX_HIP(hipGetDevice(&device));
        SX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        SX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lds ? KL : KW, SX_TILE, lds ? lds_bytes : 0));
        if (per_cu < 1) SX_FATAL("the batch kernel does not fit a compute unit");
        return per_cu * cus;
    }
    static void launch(bool lds, const Args &a, int count, int grid, size_t lds_bytes, hipStream_t s) {
        if (grid < 1 || count < 1) return;
        if (lds) {
            if (lds_bytes > SX_BATCH_LDS_BYTES) SX_FATAL("batch kernel: working set exceeds the LDS class");
            KL<<<grid, SX_TILE, lds_bytes, s>>>(a);
        } else {
            if (a.ws == nullptr || a.slice < 1) SX_FATAL("batch kernel: no workspace");
            KW<<<grid, SX_TILE, 0, s>>>(a);
        }
        SX_HIP(hipGetLastError());
    }
};
using HostEntry = Entry<BatchArgs, k_batch_solve<true>, k_batch_solve<false>>;
using DevEntry = Entry<BatchDevArgs, k_batch_solve_dev<true>, k_batch_solve_dev<false>>;
using RagEntry = Entry<BatchRagArgs, k_batch_solve_rag<true>, k_batch_solve_rag<false>>;
using StEntry = Entry<BatchStArgs, k_batch_solve_st<true>, k_batch_solve_st<false>>;
using RhsEntry = Entry<BatchRhsArgs, k_batch_solve_rhs<true>, k_batch_solve_rhs<false>>;
using RowsEntry = Entry<BatchRowsArgs, k_batch_solve_rows<true>, k_batch_solve_rows<false>>;
using ColsEntry = Entry<BatchColsArgs, k_batch_solve_cols<true>, k_batch_solve_cols<false>>;
using DropEntry = Entry<BatchDropArgs, k_batch_solve_drop<true>, k_batch_solve_drop<false>>;
using BranchEntry = Entry<BatchBranchArgs, k_batch_solve_branch<true>, k_batch_solve_branch<false>>;
using CutEntry = Entry<BatchCutArgs, k_batch_solve_cut<true>, k_batch_solve_cut<false>>;

}  // namespace

int sx_batch_resident(BatchEntry entry, bool lds, size_t lds_bytes) {
    switch (entry) {
    case BatchEntry::Dev: return DevEntry::resident(lds, lds_bytes);
    case BatchEntry::Rag: return RagEntry::resident(lds, lds_bytes);
    case BatchEntry::St: return StEntry::resident(lds, lds_bytes);
    case BatchEntry::Rhs: return RhsEntry::resident(lds, lds_bytes);
    case BatchEntry::Rows: return RowsEntry::resident(lds, lds_bytes);
    case BatchEntry::Cols: return ColsEntry::resident(lds, lds_bytes);
    case BatchEntry::Drop: return DropEntry::resident(lds, lds_bytes);
    case BatchEntry::Branch: return BranchEntry::resident(lds, lds_bytes);
    case BatchEntry::Cut: return CutEntry::resident(lds, lds_bytes);
    default: return HostEntry::resident(lds, lds_bytes);
    }
}
void sx_launch_batch_solve(bool lds, const BatchArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    HostEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchDevArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    DevEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchRagArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    RagEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchStArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    StEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchRhsArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    RhsEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchRowsArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    RowsEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchColsArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    ColsEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchDropArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    DropEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchBranchArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    BranchEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
void sx_launch_batch_solve(bool lds, const BatchCutArgs &a, int grid, size_t lds_bytes, hipStream_t s) {
    CutEntry::launch(lds, a, a.count, grid, lds_bytes, s);
}
