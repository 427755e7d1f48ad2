/*
 * simplex_hip.h -- MI355X engine extensions of the C-ABI (libsimplex_hip.so).
 *
 * Nothing here exists in the reference; it is what a benchmark, a parity test or a
 * multi-GPU launcher needs on top of the drop-in entry points (twoPhaseMethod.h).
 * Plain C types only.
 */
#ifndef SIMPLEX_HIP_H
#define SIMPLEX_HIP_H

#include "problem.h"
#include "tabular.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMPLEX_NOT_ENDED -10    /* solver.cu:77 */
#define SIMPLEX_PIVOT_CAP -11    /* opt-in pivot budget reached */
#define SIMPLEX_NUMERIC_FAIL -12 /* eligible pivot but the ratio argmin found no row */
#define SIMPLEX_HANG -13         /* fused batch: an in-kernel hand-off timed out (never expected) */
#define SIMPLEX_BAD_SHAPE -14    /* ragged device batch: a problem's dimensions lie outside the envelope */
#define SIMPLEX_BAD_STATE -15    /* state entry: a problem's saved state fails the kernel's checks */
#define SIMPLEX_MAX_GPUS 8       /* shards (GPUs) one solve can use: simplex_set_gpus, SIMPLEX_GPUS, --gpus */

/* ---- configuration ---- */
int simplex_version(void);
void simplex_set_verbose(int on);            /* reference progress lines on stdout */
/* the sweep on the matrix cores (v_mfma_f64_16x16x4f64, bit-identical to the vector chain):
 * -1 auto (matrix cores), 0 vector sweep (batches of at most 32), 1 matrix-core sweep */
void simplex_set_sweep_mfma(int mode);
/* pivots per tableau sweep (1..64; 0 = auto: 64 when the tableau has >= 4096 rows -- two stages
 * of 32, applied by the matrix-core sweep -- else 32; more than 32 only in the fused batches, one
 * shard's and the peer-memory multi-rank one, the per-pivot path caps it at 32): the pivots of a
 * batch are selected on the
 * current values (pending pivots applied on the fly) and then applied to the tableau in one
 * sweep -- the same IEEE operations in the same order as one sweep per pivot */
void simplex_set_batch(int pivots);
void simplex_set_device(int device);
/* write the reference's -D TIMER CSV (chrono.cu) into `dir` (NULL or "" = off; env
 * SIMPLEX_TIMER_DIR also enables it); benchmark mode names it benchmark_<n>_<m>.txt */
void simplex_set_timer_dir(const char *dir);

/* ---- multi-GPU: one process per GPU, RCCL communicator over xGMI ---- */
int simplex_dist_unique_id_size(void);
int simplex_dist_get_unique_id(unsigned char *out); /* rank 0; out has unique_id_size bytes */
int simplex_dist_init(int rank, int world, const unsigned char *unique_id, int device);
int simplex_dist_finalize(void);
/* single-process emulation of W row-block shards on the current device (collectives are
 * device copies); used to test the sharded path on one GPU. 0 or 1 disables. */
void simplex_set_virtual_ranks(int world);
/* ---- multi-GPU inside ONE process: the caller still makes one synchronous
 * twoPhaseMethod / solve call.  The constraint rows are split into count 512-aligned blocks, one
 * per listed device (a device may repeat); the shards hand off through peer memory (one fused
 * launch per device per batch of pivots) when a start-up self-check on the list passes, else
 * through per-pivot device copies.  Without this call the environment variable SIMPLEX_GPUS
 * decides: "N" = devices 0..N-1, or a comma list ("0,1,2,3").  count <= 1 (or no list): one
 * shard.  A device that is not visible is a fatal error (error.cu:5-12 convention). */
void simplex_set_gpus(const int *devices, int count);
/* the device list in effect (simplex_set_gpus, else SIMPLEX_GPUS); returns its length and
 * copies up to cap entries */
int simplex_gpus(int *devices, int cap);
/* run the multi-shard exchange path (tile allgather + pivot-row allreduce) even with a
 * single shard; with simplex_dist_init(.., world=1, ..) it goes through a 1-rank RCCL
 * communicator.  Test hook. */
void simplex_set_force_exchange(int on);
/* per-pivot exchange between shards: 0 auto, 1 tile-winner allgather + pivot-row allreduce,
 * 2 one allgather of tile winners together with their rows (auto: when <= 1 MiB per rank) */
void simplex_set_exchange_mode(int mode);
/* store each phase-1 artificial column as its (bit-identical) slack column: 1 on (default), 0 off */
void simplex_set_alias(int on);
/* slack compaction (default on): the slack column of a row that has never left the basis is
 * an untouched unit vector, so it is kept past the swept block of the tableau and skipped by
 * every sweep -- bit-identical results; active only when no row is negated (b >= 0) */
void simplex_set_compact(int on);
/* with slack compaction: every `every` sweeps (default 8; 0 off) the swept slack columns whose
 * slack is basic -- exact unit vectors, checked bit for bit -- are moved past the swept block too,
 * and moved back when their row leaves; bit-identical results.  On one shard, and on the row-block
 * shards of one process (virtual ranks, a SIMPLEX_GPUS / simplex_set_gpus device list), which
 * combine their per-row-block checks before any of them moves a column.  RCCL ranks with world > 1
 * and IPC-mode sessions do not deactivate. */
void simplex_set_deactivate(int every);
/* the same on the several shards of one process: 1 on (default), 0 only on one shard (the earlier
 * rule; for A/B runs and for bisecting on multi-GPU hardware) */
void simplex_set_deactivate_shards(int on);
/* one shard: run each batch of pivots as ONE resident launch (ratio tiles + objective-row tiles
 * handing off through write-through records) instead of two launches per pivot;
 * -1 auto (default: when the grid fits the device), 0 off */
void simplex_set_fused(int mode);
/* several shards: run each batch as ONE launch per rank whose ranks hand off through peer
 * memory (xGMI; virtual shards: the same device) instead of per-pivot RCCL calls; -1 auto
 * (default: RCCL ranks when the start-up self-check in simplex_dist_init passed), 0 off,
 * 1 force (virtual shards: only with 1; all ranks' batches as one launch, or with
 * simplex_set_mr_single_launch(0) one launch per rank for W <= 3) */
void simplex_set_p2p(int mode);
/* 1 when the peer-memory fused path passed simplex_dist_init's self-check on every rank */
int simplex_p2p_ready(void);
/* how the shards of this process (RCCL ranks, or the SIMPLEX_GPUS device list) passed their
 * start-up self-check against a one-shard solve of the same instance: 2 peer-memory fused batches,
 * 1 the per-pivot exchange, 0 neither (every solve then runs on one device: RCCL ranks each solve
 * alone, a device list on its first device), -1 not checked (yet) or one shard */
int simplex_multi_gpu_mode(void);
/* wall time (s) of the last twoPhaseMethod call's two pivot loops (solve calls): out[0] phase 1,
 * out[1] phase 2 -- the reference's TIMER CSV reports the two phases separately */
void simplex_last_phase_seconds(double *out);
/* the last twoPhaseMethod call's final objective row d[0, N) in logical columns (N = 1+n+m after
 * phase 2, 1+n+2m when phase 1 ended the solve): copies min(N, cap) entries, returns N.  After a
 * FEASIBLE solve, d[1+n+i] = y_i (the dual of constraint i, also for the rows negated by the b < 0
 * quirk, twoPhaseMethod.cu:100-111) and d[1+j] = (A^T y)_j - c_j: a dual certificate */
long long simplex_last_objective_row(double *out, long long cap);
/* the sweep's grid: waves x (blocks resident on the device) blocks (default 1; <= 0 resets) */
void simplex_set_update_waves(double waves);
/* new engines' tableau layout: plain row-major rows (0), the two-region layout when aliasing and
 * m > 4096 (1, default), or region A forced to hold `mode` slack positions (>= 2,
 * test hook) */
void simplex_set_regions(int mode);
/* virtual shards with the peer-memory batch: every rank's batch in one launch (1, default) or one
 * launch per rank on its own stream (0; needs as many hardware queues running at once) */
void simplex_set_mr_single_launch(int on);

/* the pending pivot rows U (written by peer ranks in the multi-rank batch) in fine-grained memory:
 * -1 auto (when the shards span devices, default), 1 always (test hook: the one-GPU cost and
 * parity of that path), 0 never; 2 (test hook): uncached memory for exchanging shards, the
 * allocation of the round-4/5 divergence */
void simplex_set_fine_pivot_rows(int mode);
/* multi-rank fused batches with the objective row replicated: every rank runs every objective
 * tile (decides the entering variable and forms the whole pivot row itself), so a pivot's only
 * cross-rank hand-offs are the ratio tiles' winners and the leaving row read from its owner
 * (DESIGN.md §5.2): -1 auto (when the shards span devices, default), 1 always (when the grid of
 * slots + every objective tile per rank fits; else the split objective), 0 never (each rank runs
 * its share of the objective tiles and the records go to every rank) */
void simplex_set_replicated_objective(int mode);
/* new engines' tableau storage inside each region: -1 default (blocks of 4 rows x 4 columns in
 * 16-row strips, unless the environment sets SIMPLEX_BLOCKED=0), 1 blocked, 0 plain row-major
 * (callers' tableaux, tabular.h, are always row-major) */
void simplex_set_blocked(int mode);

/* ---- fault handling and test hooks ---- */
/* a fused batch whose in-kernel hand-off wait times out (SIMPLEX_HANG, never expected) is
 * undone and re-run on the per-pivot path; this counts such recoveries in the process */
long long simplex_hang_recoveries(void);
long long simplex_fused_batches(void);           /* fused batch launches in the process */
/* diagnostic: before every sweep of a multi-shard engine of this process (virtual shards, a
 * SIMPLEX_GPUS list), compare every shard's pending pivot rows U with shard 0's bit for bit and
 * count (and print the first) mismatches -- 1 on, 0 off (default; SIMPLEX_CHECK_PIVOT_ROWS=1 also
 * turns it on).  Synchronous per batch: for tests and diagnosis, not for timing */
void simplex_set_check_pivot_rows(int on);
long long simplex_pivot_row_mismatches(void);    /* mismatches counted in the process */
/* test hook: make the n-th fused batch from now abort as if a wait had timed out (-1 off) */
void simplex_set_hang_inject(long long batches);
/* ... at which slot of that batch: -1 (default) before it starts; s >= 0: the batch runs s
 * pivots (the objective row already updated by them) and then one block leaves it, so the others
 * time out inside the batch */
void simplex_set_hang_inject_slot(int slot);
/* test hook: batch id of the next engine's first batch (1 .. 32767; ids wrap at 32768) */
void simplex_set_first_batch_id(unsigned int id);

/* ---- extended drop-in entry ---- */
/* twoPhaseMethod + final basis (base_out[m]) and per-phase pivot counts (pivots_out[2]);
 * max_pivots < 0 = no cap (parity mode), else per-phase cap (status SIMPLEX_PIVOT_CAP).
 * It returns the engine-only statuses (SIMPLEX_PIVOT_CAP, SIMPLEX_NUMERIC_FAIL, SIMPLEX_HANG)
 * as such; twoPhaseMethod and solve keep the reference contract (0/-1/-2/-3, solve 0/-2) and
 * treat NUMERIC_FAIL and HANG as fatal errors (print, exit; error.cu:5-12). */
int twoPhaseMethodEx(problem_t *problem, double *solution, double *optimalValue, int *base_out,
                     long long *pivots_out, long long max_pivots);

/* ---- batched solve: many small LPs in one resident launch ---- */
/* every problem's twoPhaseMethodEx result, solved together; per-problem outputs:
 * status_out[count], opt_out[count], pivots_out[count][2]; solutions[k] (vars doubles) and
 * base_out[k] (constraints ints) may be NULL as arrays or per entry.  Returns 0, <0 on bad arguments.
 * A problem whose working set fits a compute unit's LDS, or a 4 MiB slice of device memory, is
 * solved whole by one workgroup; larger ones go through the engine inside the same call, so every
 * shape is accepted.  Results are bit-identical to twoPhaseMethodEx either way (solutions[k] and
 * opt_out[k] are written only for a FEASIBLE problem; max_pivots as in twoPhaseMethodEx).  Runs on
 * the current device (simplex_set_device) and ignores the shard settings (SIMPLEX_GPUS,
 * simplex_set_gpus, virtual ranks); count == 0 is valid.  What simplex_last_objective_row and
 * simplex_last_phase_seconds report after a batch call is unspecified. */
int simplex_solve_batch(problem_t *const *problems, int count, long long max_pivots, int *status_out,
                        double *const *solutions, double *opt_out, int *const *base_out, long long *pivots_out);
/* where a problem of this shape would run: 2 LDS-resident, 1 workspace-resident, 0 engine; host arithmetic only */
int simplex_batch_class(int n, int m);
/* of the last simplex_solve_batch call: out[0] LDS-resident, out[1] workspace-resident, out[2] engine
 * (too large), out[3] evicted to the engine after exhausting the resident budget (these are also
 * counted in out[0] or out[1], where they started) */
void simplex_batch_counts(long long out[4]);
/* resident pivot budget per phase (0 = default formula, 64 + 16 (n + m)); test hook and safety valve:
 * a resident problem that needs more pivots is re-solved from scratch by the engine, uncapped */
void simplex_set_batch_budget(long long pivots);

/* ---- device-resident batched solve: device arrays in, device arrays out, no host copy ---- */
/* count problems of ONE shape (n variables x m constraints, simplex_batch_class(n, m) 2 or 1; larger
 * shapes belong to simplex_solve_batch), read in place from device memory through element strides
 * and solved by the same resident workgroups; every per-problem result is written to dense device
 * arrays by the kernel itself.  The call only enqueues on `stream` (two small memsets and one
 * launch) on the current device: it allocates nothing, copies nothing, never synchronises and keeps
 * no state, so calls on different streams with different outputs and workspaces are independent.
 * The inputs are not written; outputs and workspace must not overlap them or each other.
 * Element strides may be negative: A, b and c are the addresses of the logical first elements (the
 * last ones in memory along a reversed dimension) and A[k][i][j] is read at
 * A + k * A_sb + i * A_sr + j * A_sc whatever the signs.  The same holds for the ragged entry,
 * simplex_solve_device and simplex_dev_build_phase1_device; only a stride of 0 is refused (-4).
 * Per problem the results are twoPhaseMethodEx's: status, pivots (phase 1, phase 2) and base as
 * there; for a FEASIBLE problem opt and x bit for bit, for any other status opt is a quiet NaN and
 * x is all +0.0 (never stale memory).  objrow[k] is what simplex_last_objective_row reports for
 * that problem: row_width[k] = 1+n+m entries after phase 2, 1+n+2m when phase 1 ended the solve,
 * and +0.0 from row_width[k] up to 1+n+2m.
 * A problem that exhausts the resident pivot budget (simplex_set_batch_budget) is NOT re-solved
 * here: it is left with status SIMPLEX_NOT_ENDED, opt NaN, x zero and row_width 0, and counted in
 * *evicted; the caller re-solves it with twoPhaseMethodEx (no other path gives NOT_ENDED), or
 * keeps its state and continues it on the device with simplex_solve_batch_device_state (below).
 * Shard settings are ignored, as in simplex_solve_batch. */
typedef struct {
    int n, m, count;                       /* every problem n variables x m constraints */
    const double *A; long long A_sb, A_sr, A_sc;   /* element strides: batch, row (constraint), column (variable) */
    const double *b; long long b_sb, b_si;
    const double *c; long long c_sb, c_sj;
    long long max_pivots;                  /* as twoPhaseMethodEx */
    /* outputs, device memory, dense: */
    int *status;          /* [count] */
    long long *pivots;    /* [count][2] */
    double *opt;          /* [count] */
    double *x;            /* [count][n]        or NULL */
    int *base;            /* [count][m]        or NULL */
    double *objrow;       /* [count][1+n+2m]   or NULL */
    int *row_width;       /* [count]           or NULL */
    int *evicted;         /* [1]: problems left SIMPLEX_NOT_ENDED by the resident budget */
    void *workspace; long long workspace_bytes;   /* 16-byte aligned; simplex_batch_device_workspace bytes */
    void *stream;         /* hipStream_t; NULL = the null stream */
} simplex_batch_device_t;

/* bytes of workspace a call of this shape and count needs on the current device (a header with the
 * work counter; for class 1 also one working-set slice per resident workgroup); -1 for count < 0,
 * -3 for n < 1, m < 1 or a class-0 shape -- both decided before any device is touched */
long long simplex_batch_device_workspace(int n, int m, int count);
/* returns 0 (count == 0: nothing is launched), -1 args NULL or count < 0, -3 shape (as above),
 * -2 a required pointer is NULL (A, b, c, status, pivots, opt, evicted), -4 a stride of 0 on a
 * dimension longer than 1, -5 workspace NULL, misaligned or too small */
int simplex_solve_batch_device(const simplex_batch_device_t *args);

/* ---- ragged device batch: per-problem shapes inside one padded envelope ---- */
/* simplex_solve_batch_device with args->n x args->m as an ENVELOPE: the input and output arrays keep
 * its shapes and strides, and problem k is the LP on the leading block A[k][0..m_k[k])[0..n_k[k]),
 * b[k][0..m_k[k]), c[k][0..n_k[k]).  n_k and m_k are int arrays of count entries in device memory.
 * No element outside a problem's block is read (the padding may hold anything), and problem k gets
 * twoPhaseMethodEx's result for that n_k[k] x m_k[k] problem, bit for bit; solving a zero-padded
 * problem instead does not give it.  max_pivots, the resident budget (by default that of the
 * problem's own shape) and eviction work as in simplex_solve_batch_device.
 * Outputs, in the envelope's dense shapes: x[k][n_k[k]..n) is +0.0; base[k][m_k[k]..m) is -1, and
 * base[k][i] is in the problem's own numbering (< n_k structural, n_k + i slack, n_k + m_k + i
 * artificial); objrow[k] is laid out in ENVELOPE columns -- [0] the objective, [1 + j] the structural
 * entry j < n_k, [1 + n + i] the slack entry (the dual y_i) i < m_k, [1 + n + m + i] the artificial
 * entry i < m_k when phase 1 ended the solve, +0.0 everywhere else -- so column arithmetic on the
 * envelope's n and m holds for every problem; row_width[k] stays the problem's own logical width
 * (1+n_k+m_k, 1+n_k+2m_k, or 0 when evicted).  With n_k[k] == n and m_k[k] == m everything is
 * simplex_solve_batch_device's.
 * The host cannot see the dimensions without a synchronisation, so the kernel tests them before it
 * indexes anything with them: n_k[k] < 1, m_k[k] < 1, n_k[k] > n or m_k[k] > m gives problem k the
 * status SIMPLEX_BAD_SHAPE, pivots 0, opt NaN, x zero, base -1, a zero row and row_width 0; the other
 * problems of the call are not affected.
 * order (device, count ints) or NULL: the j-th problem a workgroup takes from the work counter is
 * order[j] (NULL: j).  Larger problems first keep the long ones out of the tail.  It must be a
 * permutation of 0..count-1 (the caller's contract); an entry outside that range is skipped, and
 * results do not depend on the order.
 * The workspace is simplex_batch_device_workspace(n, m, count) bytes, the envelope's.  Returns
 * simplex_solve_batch_device's codes, -2 also for a NULL n_k or m_k.  Like that entry the call only
 * enqueues two small memsets and one launch on `stream`. */
int simplex_solve_batch_device_ragged(const simplex_batch_device_t *args, const int *n_k, const int *m_k,
                                      const int *order /* or NULL */);

/* ---- device batch state: resume capped or evicted problems, warm-start new costs ---- */
/* simplex_solve_batch_device that can keep each problem's final working set on the device and start
 * from a kept one.  A state is dense per problem and belongs to one shape (n, m) and count:
 * T holds the 1+n+m stored columns b | structural | slack (in phase 1 the artificial block is the
 * slack block bit for bit, so it is not kept), d the objective row at the full width 1+n+2m
 * (entries [1+n+m, 1+n+2m) are +0.0 in a phase-2 state), base the basis, phase where the problem
 * stands (1: in phase 1, 2: in phase 2, 0: no state) and pivots the pivots done so far per phase.
 *
 * in == NULL: a fresh solve -- exactly simplex_solve_batch_device, every output bit for bit -- whose
 * final working sets are written to out.
 * in != NULL: a resume.  args->A and args->b are not read and may be NULL; args->c is required (it is
 * read when a phase-1 state reaches phase 2, and for recost) and only its strides are checked.  Each
 * problem's T, d and base are loaded instead of being built, and the two-phase loop is re-entered:
 * a phase-1 state continues phase 1 at pivots[0], and when that ends FEASIBLE runs phase 2 from 0
 * with args->c; a phase-2 state continues phase 2 at pivots[1], or with recost != 0 (the warm start
 * for new costs on the same constraints) restarts phase 2 from pivot 0 on the saved tableau and
 * basis with d[0] = +0.0, d[1+j] = -c[j], the slack entries +0.0, made canonical for the basis;
 * pivots[0] is kept.  No outcome has a case of its own: a state that ended FEASIBLE, UNBOUNDED,
 * INFEASIBLE, DEGENERATE or NUMERIC_FAIL gives that status again with no new pivot.
 * max_pivots caps each phase's total, saved plus new, as one call would: a capped call followed by a
 * resume with -1 is the uncapped solve, bit for bit, in every output and in the state.  The resident
 * budget (simplex_set_batch_budget) counts the pivots of THIS call per phase, so a problem left
 * SIMPLEX_NOT_ENDED progresses with every resume; it is left with the state a cap at the same count
 * leaves, and resumed here instead of re-solved by twoPhaseMethodEx.
 * out == NULL: the state is not kept.  out may equal in, member for member (a workgroup owns its
 * problem and has loaded all of it before it writes); any other overlap is the caller's error.
 * The host cannot see a state, so the kernel tests it before it indexes anything with it: phase must
 * be 1 or 2, both pivot counts >= 0, every base[i] in [0, n+2m) in phase 1 and [0, n+m) in phase 2.
 * A problem that fails gets the status SIMPLEX_BAD_STATE, pivots 0, opt NaN, x zero, base -1, a zero
 * row, row_width 0 and out->phase 0 (nothing else of out is written for it); the other problems of
 * the call are not affected.
 * Returns simplex_solve_batch_device's codes; -2 also for a NULL member of a non-NULL state struct
 * and for a NULL c with in != NULL.  The workspace is simplex_batch_device_workspace(n, m, count).
 * Like that entry the call only enqueues two small memsets and one launch on `stream`. */
typedef struct {
    double *T;          /* [count][m][1+n+m]  stored columns b | structural | slack, row-major, dense */
    double *d;          /* [count][1+n+2m]    objective row */
    int *base;          /* [count][m] */
    int *phase;         /* [count]            1: in phase 1, 2: in phase 2, 0: no state (3: see ..._rhs) */
    long long *pivots;  /* [count][2]         pivots done so far in phase 1, phase 2 */
} simplex_batch_state_t;
int simplex_solve_batch_device_state(const simplex_batch_device_t *args,
                                     const simplex_batch_state_t *in /* NULL: fresh solve */,
                                     const simplex_batch_state_t *out /* NULL: state not kept */, int recost);

/* ---- device batch state: a new right-hand side (dual simplex) ---- */
/* Re-solve kept states for a new b, or resume states such a call left.  A state's phase has one more
 * value here: 3, phase 2's tableau inside the dual loop (dual feasible, primal infeasible), with
 * phase 2's basis range [0, n+m).  simplex_solve_batch_device_state keeps rejecting 3 with
 * SIMPLEX_BAD_STATE: a primal resume of a primal-infeasible tableau would be wrong.
 *
 * rerhs == 0: a resume.  Phase-1 and phase-2 states behave as in simplex_solve_batch_device_state(args,
 * in, out, 0), bit for bit; a phase-3 state re-enters the dual loop at pivots[1].  args->A and args->b
 * are not read and may be NULL.
 * rerhs != 0: args->A, args->b and args->c are required; b is the new right-hand side and c must be
 * the costs the state was solved with.  Per problem:
 *   cold start -- the state is in phase 1, or its objective row is not dual feasible (the eps-argmin of
 *   d[1 .. 1+n+m) compares below zero: a state that ended UNBOUNDED or was capped in phase 2): the
 *   problem is built from A, b, c and solved exactly as simplex_solve_batch_device does, every output
 *   bit for bit, pivots counted from (0, 0);
 *   warm start -- otherwise.  The kept slack block is S = B^-1 D (D the negation of the rows built with
 *   b_i < 0, applied to the slack entry too), so T[i][0] = sum_k S[i][k] b[k] and d[0] = sum_i d[1+n+i]
 *   b[i], each summed in ascending order by fma from +0.0 in 512-element blocks, the block sums added
 *   left to right; pivots[0] is kept and pivots[1] = 0.  Then the dual loop at width 1+n+m, counting
 *   into pivots[1]: stop with SIMPLEX_PIVOT_CAP at max_pivots; the leaving row r is the eps-argmin of
 *   T[i][0]; the loop is left when that minimum does not compare below zero; SIMPLEX_INFEASIBLE when no
 *   column j has -T[r][j] >= eps; the resident budget (SIMPLEX_NOT_ENDED); the entering variable e is
 *   the eps-argmin of d[1+j] / -T[r][1+j] over the columns with compare(-T[r][1+j], 0) > 0
 *   (SIMPLEX_NUMERIC_FAIL if there is none); then the primal loop's update with the pivot T[r][1+e].
 *   Behind the dual loop phase 2 continues at the same count -- it makes no pivot while the row is
 *   within eps -- and gives the final status.
 * What ends inside the dual loop (cap, budget, INFEASIBLE, NUMERIC_FAIL) leaves out->phase 3, anything
 * later 2.  As in the state entry no outcome has a case of its own: a phase-3 state that ended
 * INFEASIBLE gives INFEASIBLE again without a pivot, and a capped call resumed with -1 is the uncapped
 * call bit for bit.  x, opt, objrow and row_width (1+n+m in phases 2 and 3) follow
 * simplex_solve_batch_device's rules.
 * Returns simplex_solve_batch_device_state's codes, decided before any device is touched; -2 also for a
 * NULL in and, with rerhs, a NULL A or b; the strides of A and b are checked only when they are read.
 * The workspace is simplex_batch_device_workspace(n, m, count); the call only enqueues two small
 * memsets and one launch on `stream`. */
int simplex_solve_batch_device_rhs(const simplex_batch_device_t *args, const simplex_batch_state_t *in /* required */,
                                   const simplex_batch_state_t *out /* NULL: state not kept; may equal in */,
                                   int rerhs);

/* ---- device batch state: new constraint rows (cuts, branching) ---- */
/* Grow kept states of shape (n, m0) by `added` = q constraint rows to (n, m = m0 + q) and re-solve them.
 * args describes the GROWN problem: args->m = m, A [count][m][n], b [count][m], c [count][n] through any
 * non-zero strides, every output in the grown shape, the workspace simplex_batch_device_workspace(n, m,
 * count).  Rows 0 .. m0 of A and b, and c, must be what `in` was solved with (the caller's contract).
 * `in` has the shape (n, m0): T [count][m0][1+n+m0], d [count][1+n+2 m0], base [count][m0]; `out` the
 * grown one.  Write Ns0 = 1+n+m0 and Ns = 1+n+m.
 * The kernel tests a state against the in-state's own shape: phase in {1, 2, 3}, both pivot counts >= 0,
 * base[i] in [0, n+2 m0) in phase 1 and in [0, n+m0) otherwise; a failure gives SIMPLEX_BAD_STATE with
 * simplex_solve_batch_device_state's cleared outputs and out->phase 0.
 * A state in phase 2 or 3 is loaded into the grown working set: old row i is T_in[i][0 .. Ns0) followed by
 * q entries of +0.0; d[0 .. Ns0) is the state's and d[Ns0 .. 1+n+2m) is +0.0; base[0 .. m0) is the state's
 * and base[m0+t] = n+m0+t.
 *   cold start -- the state is in phase 1, or the eps-argmin of the grown d[1 .. Ns) compares below zero:
 *   the problem is built from A, b, c and solved exactly as simplex_solve_batch_device does on the grown
 *   problem, every output bit for bit, pivots counted from (0, 0);
 *   warm start -- otherwise.  For each new row t < q the raw row is R[0] = b[m0+t], R[1+j] = A[m0+t][j],
 *   R[1+n+k] = (k == m0+t) ? 1.0 : +0.0, the multipliers are f_i = base[i] < n ? A[m0+t][base[i]] : +0.0
 *   for i < m0, and the stored entry T[m0+t][j], j in [0, Ns), starts at R[j] and takes fma(-f_i, T[i][j], .)
 *   for i = 0, 1, .., m0-1 in that order.  The new rows do not depend on each other, d is unchanged,
 *   pivots[0] is kept and pivots[1] = 0.  Then simplex_solve_batch_device_rhs's dual loop from 0 at width
 *   Ns and phase 2 at the same count, with that entry's statuses and its phase-3 rule.  The basic
 *   columns of a new row come out as the chain computes them; they are not forced to zero.
 * The grown state is a state of simplex_solve_batch_device_rhs for the shape (n, m): a resume (rerhs == 0)
 * continues a capped dual loop, and a new right-hand side [m] is valid on it.
 * Returns simplex_solve_batch_device_rhs's codes, decided before any device is touched; -2 also for a NULL
 * in, A, b or c and for an out that shares a member pointer with in (the shapes differ, so in place is
 * impossible); -3 also for added < 1 or added >= m.  The call only enqueues two small memsets and one
 * launch on `stream`. */
int simplex_solve_batch_device_rows(const simplex_batch_device_t *args,
                                    const simplex_batch_state_t *in /* required: shape (n, m - added) */,
                                    const simplex_batch_state_t *out /* NULL: not kept; shape (n, m) */, int added);

/* ---- device batch state: new variable columns (column generation) ---- */
/* Grow kept states of shape (n0, m) by `added` = p structural columns to (n = n0 + p, m) and re-solve them.
 * args describes the GROWN problem: args->n = n, A [count][m][n], b [count][m], c [count][n] through any
 * non-zero strides, every output in the grown shape, the workspace simplex_batch_device_workspace(n, m,
 * count).  Columns 0 .. n0 of A and c, and b, must be what `in` was solved with (the caller's contract).
 * `in` has the shape (n0, m): T [count][m][1+n0+m], d [count][1+n0+2m], base [count][m]; `out` the grown
 * one.  Write Ns0 = 1+n0+m and Ns = 1+n+m.
 * The kernel tests a state against the in-state's own shape: phase in {1, 2, 3}, both pivot counts >= 0,
 * base[i] in [0, n0+2m) in phase 1 and in [0, n0+m) otherwise; a failure gives SIMPLEX_BAD_STATE with
 * simplex_solve_batch_device_state's cleared outputs and out->phase 0.
 * A state in phase 2 or 3 is loaded into the grown working set, the structural block growing in the
 * middle: stored column j < 1+n0 stays at j, slack column 1+n0+k moves to 1+n+k, in T and in d;
 * d[Ns .. 1+n+2m) is +0.0; a basis entry base[i] >= n0 (a slack) becomes base[i] + p.  Then, for t < p,
 *   T[i][1+n0+t] = sum_k S[i][k] A[k][n0+t]   and   d[1+n0+t] = (sum_i y_i A[i][n0+t]) - c[n0+t],
 * S the loaded slack block and y the loaded slack entries of d, each sum as simplex_solve_batch_device_rhs
 * takes S b': ascending by fma from +0.0 in 512-element blocks, the block sums added left to right; the
 * subtraction of c is one rounded operation behind the sum.  d[0], the right-hand-side column and the old
 * columns are unchanged; pivots[0] is kept and pivots[1] = 0.
 *   a phase-2 state is always warm: the old basis stays primal feasible, so phase 2 runs from count 0
 *   at width Ns, whatever the state's old status was (a capped or UNBOUNDED state simply continues);
 *   a phase-3 state is warm while the eps-argmin of the grown d[1 .. Ns) does not compare below zero:
 *   simplex_solve_batch_device_rhs's dual loop from 0, then phase 2 at the same count, with that
 *   entry's statuses and its phase-3 rule -- a state that an infeasible row or right-hand side left
 *   inside the dual loop is rescued by a column with a negative entry in the blocking row;
 *   cold start -- a phase-1 state, or a phase-3 state whose grown row is not dual feasible: the problem
 *   is built from A, b, c and solved exactly as simplex_solve_batch_device does on the grown problem,
 *   every output bit for bit, pivots counted from (0, 0).
 * The grown state is a state of simplex_solve_batch_device_rhs and of simplex_solve_batch_device_rows for
 * the shape (n, m): a resume, a new right-hand side, further rows and further columns are valid on it.
 * Returns simplex_solve_batch_device_rows's codes, decided before any device is touched; -2 also for a
 * NULL in, A, b or c and for an out that shares a member pointer with in; -3 also for added < 1 or
 * added >= n.  The call only enqueues two small memsets and one launch on `stream`. */
int simplex_solve_batch_device_cols(const simplex_batch_device_t *args,
                                    const simplex_batch_state_t *in /* required: shape (n - added, m) */,
                                    const simplex_batch_state_t *out /* NULL: not kept; shape (n, m) */, int added);

/* ---- device batch state: rows or columns taken out again (cut purging, undone branches) ---- */
/* Reduce kept states by `dropped` = q constraint rows (kind 0: shape (n, m + q) to (n, m)) or q structural
 * columns (kind 1: shape (n + q, m) to (n, m)) and re-solve them.  args describes the REDUCED problem:
 * A [count][m][n], b [count][m], c [count][n] through any non-zero strides -- what `in` was solved with,
 * with the named rows or columns deleted (the caller's contract); they are read only when a problem goes
 * cold -- and every output in the reduced shape.  `in` has the in-state's shape (n_in, m_in), `out` the
 * reduced one.  idx [count][q], dense int32 on the device, holds problem k's own indices: strictly
 * ascending, in [0, m_in) or [0, n_in); a list that is not gets what a state that fails its range test
 * gets: SIMPLEX_BAD_STATE, simplex_solve_batch_device_state's cleared outputs and out->phase 0.
 * The kernel works in the in-state's shape, so the class (simplex_batch_class) and the workspace
 * (simplex_batch_device_workspace(n_in, m_in, count)) are that shape's.  A state is tested against its own
 * shape as simplex_solve_batch_device_rhs tests it, then loaded, and the drops are applied one at a time
 * in descending index order, each at the shape the earlier ones left:
 *   row r (slack n + r, stored column 1 + n + r): a basic slack's row and column are deleted without
 *   arithmetic.  A nonbasic slack is first forced into the basis: with an entry >= eps in its column the
 *   leaving row is the primal ratio eps-argmin; else with an entry <= -eps the same argmin over the
 *   negated column (the slack leaves the problem, so it may move down; the pivot element is negative);
 *   else the problem is cold.  The pivot is the primal loop's; then the slack's row and column go.
 *   column j: a nonbasic column is deleted without arithmetic.  One that is basic in row i is forced out
 *   by a dual pivot on that row: with s = +1 if T[i][0] does not compare below zero, else -1, the
 *   entering variable is the eps-argmin of d[1 + t] / (s T[i][1 + t]) over the other variables t with
 *   s T[i][1 + t] >= eps; without a candidate the problem is cold.
 *   Basis entries above a deleted variable go down by one.
 * Warm or cold: a phase-1 state is cold; a phase-3 state with row drops is warm only if every dropped
 * slack is basic; column drops of which one is basic are warm only while the eps-argmin of the loaded
 * d[1 .. 1 + n_in + m_in) does not compare below zero (tested once, before the first drop).  A cold
 * problem is built from A, b, c and solved exactly as simplex_solve_batch_device does on the reduced
 * problem, every output bit for bit, pivots counted from (0, 0).
 * Counts: pivots[0] is kept and pivots[1] starts at f, the number of forced pivots, which belong to the
 * load: neither max_pivots nor the resident budget counts them.  Behind the drops a phase-3 state, or a
 * column drop with f > 0, runs simplex_solve_batch_device_rhs's dual loop from f and then phase 2 at the
 * same count, with that entry's statuses and phase-3 rule; everything else runs phase 2 from f.
 * The reduced state is a state of every state entry for the shape (n, m).
 * Returns simplex_solve_batch_device_rows's codes, decided before any device is touched; -2 also for a
 * NULL in, A, b, c or idx and for an out that shares a member pointer with in; -3 also for kind outside
 * {0, 1}, dropped < 1, a reduced dimension below 1 and an in-state's shape of class 0.  The call only
 * enqueues two small memsets and one launch on `stream`. */
int simplex_solve_batch_device_drop(const simplex_batch_device_t *args,
                                    const simplex_batch_state_t *in /* required: the in-state's shape */,
                                    simplex_batch_state_t *out /* NULL: not kept; shape (n, m) */,
                                    int kind /* 0: constraint rows, 1: structural columns */,
                                    int dropped /* q >= 1, the same for every problem */,
                                    const int *idx /* device, int32 [count][dropped], dense */);

/* ---- device batch state: branching (many children per kept parent, bound rows) ---- */
/* Branch kept states: child k continues the kept state of problem parent[k] with one more bound row.
 * args->n, args->m and args->count = C are the CHILDREN's shape and number: every output, `out` and the
 * workspace simplex_batch_device_workspace(n, m, C) are that shape's.  The problem data are not repeated
 * per child: args->A, b and c hold `roots` = R problems of mA = m - depth rows, A [R][mA][n], b [R][mA],
 * c [R][n] through the struct's strides (a batch stride may be 0 only when R == 1), read in place, and
 * child k is the LP of problem root[k] followed by the depth = q rows
 *   coef[k][t] * x_{var[k][t]} <= rhs[k][t],   t = 0 .. q-1,
 * given as triples, dense and row-major on the device.  The first q-1 of them must be the rows the state of
 * parent[k] was solved with, behind root[k]'s own (the caller's contract, as with
 * simplex_solve_batch_device_rows); the last one is new.  `in` holds `parents` = P problems of shape
 * (n, m-1); it is only read, so any number of children may name one parent.
 * Per child the call is simplex_solve_batch_device_rows with added = 1 on the explicit inputs -- the
 * in-state of problem parent[k], and the dense grown A whose bound rows hold coef at column var and +0.0
 * elsewhere, with b ending in rhs: status, pivots, opt, x, base, objrow, row_width and the out-state are
 * that call's bit for bit, and so are its warm and cold decisions.
 *   cold start -- the parent is in phase 1, or the eps-argmin of its d[1 .. 1+n+m-1) followed by +0.0
 *   compares below zero: the phase-1 tableau of root[k]'s rows plus all q bound rows is built and solved as
 *   simplex_solve_batch_device does, a row with compare(b_i, 0) < 0 negated across all its entries;
 *   warm start -- otherwise.  With v = var[k][q-1], the raw row is R[0] = rhs[k][q-1], R[1+j] = (j == v) ?
 *   coef[k][q-1] : +0.0, R[1+n+i] = (i == m-1) ? 1.0 : +0.0, the multipliers are f_i = (base[i] == v) ?
 *   coef[k][q-1] : +0.0, and T[m-1][j] starts at R[j] and takes fma(-f_i, T[i][j], .) for i = 0 .. m-2 in
 *   that order, the whole chain (the zero multipliers decide signed zeros).  pivots[0] is kept,
 *   pivots[1] = 0; then the dual loop from 0 and phase 2 at the same count.
 * Tested on the device before anything is indexed with the values: parent[k] in [0, P), root[k] in [0, R),
 * every var[k][t] in [0, n), then the in-state of parent[k] as simplex_solve_batch_device_rows tests it
 * against the shape (n, m-1).  A child that fails gets SIMPLEX_BAD_STATE with
 * simplex_solve_batch_device_state's cleared outputs and out->phase 0; the other children are not
 * affected.  coef and rhs are data, as the entries of A are.
 * The out-state is a state of every state entry and of this one for the shape (n, m); a child stopped
 * inside the dual loop is kept in phase 3.  With out NULL no state is kept: the form for strong branching,
 * where max_pivots bounds each probe; a probe stopped by it inside the dual loop has opt NaN, and its
 * dual bound is objrow[k][0].
 * Returns, decided before any device is touched: -1 args NULL or count < 0; -3 a shape (n, m) of class 0,
 * depth < 1, depth >= m, roots < 1 or parents < 1; 0 for count == 0; -2 br or one of its five arrays
 * NULL, a required output NULL, in NULL or incomplete, out incomplete or sharing a member pointer with
 * in, A, b or c NULL; -4 a zero stride of A, b or c along a dimension longer than 1 (the batch dimension
 * has length R, the row dimension mA); -5 the workspace.  The call only enqueues two small memsets and one
 * launch on `stream`. */
typedef struct {
    int roots;          /* R: problems held in args->A, b, c */
    int parents;        /* P: problems held in the in-state */
    int depth;          /* q >= 1: bound rows per child; the last one is new */
    const int *root;    /* [count]      child k's problem is root[k] */
    const int *parent;  /* [count]      child k continues in-state problem parent[k] */
    const int *var;     /* [count, q]   dense, row-major */
    const double *coef; /* [count, q] */
    const double *rhs;  /* [count, q] */
} simplex_batch_branch_t;

int simplex_solve_batch_device_branch(const simplex_batch_device_t *args,
                                      const simplex_batch_state_t *in /* required: P problems of shape (n, m - 1) */,
                                      const simplex_batch_state_t *out /* NULL: not kept; count problems of shape (n, m) */,
                                      const simplex_batch_branch_t *br);

/* Gomory mixed-integer cuts from kept states: simplex_solve_batch_device_rows whose `cuts` = q new rows are
 * not given but derived, per problem, from the kept optimum, written out in the caller's variables, and
 * added in the same launch.  args is the grown shape (n, m) and count as there; `in` has the shape (n, m0),
 * m0 = m - q, and `out` the grown one.  args->A [count][m0][n] and args->b [count][m0] hold the rows the
 * in-state was solved with and are only read, through the struct's strides (a batch stride may be 0 only
 * when count == 1).  The new rows are outputs: cut_A [count][q][n] and cut_b [count][q], each through its
 * own element strides; they may be rows m0 .. m of the arrays args->A and args->b point into, and nothing
 * the call writes is read back from memory by it.  eps and compare are macro.h's; every fused operation
 * below is one fma, nothing else is contracted.  Per problem k:
 *   state tests -- simplex_solve_batch_device_rows's, against (n, m0).  A problem that fails gets
 *   SIMPLEX_BAD_STATE, cleared outputs, out->phase 0, cut_row[k][.] = -1 and cut_A, cut_b of +0.0.
 *   usable -- the state is in phase 2 and that entry's warm test holds (the eps-argmin of d[1 .. 1+n+m0)
 *   followed by q of +0.0 does not compare below zero): a kept optimum.  Every cut of a problem that is
 *   not usable is the null row.
 *   cut t = 0 .. q-1, source row -- row i < m0 is eligible when v = base[i] < n, integer[k][v] != 0, with
 *   t0 = T[i][0] and f0 = t0 - floor(t0) both f0 >= away and 1.0 - f0 >= away, and no cut t' < t took it.
 *   Its key is -fmin(f0, 1.0 - f0), that of any other row DBL_MAX.  With row NULL the source row r is the
 *   eps-argmin of the keys by the reference's tree, and there is no cut when the minimum is DBL_MAX; else
 *   r = row[k][t] if that lies in [0, m0) and is eligible, and there is no cut otherwise.  cut_row[k][t] = r,
 *   or -1.
 *   the null row, for no cut -- cut_A[k][t][j] = +0.0 for all j and cut_b[k][t] = +0.0: 0 x <= 0 is valid, so
 *   every problem of the call grows to the same shape; simplex_solve_batch_device_drop takes it out again.
 *   coefficients of source row r over the stored columns jj in [0, n+m0) -- f0 as above, rho = f0 /
 *   (1.0 - f0), alpha = T[r][1+jj].  g_jj = +0.0 when jj is one of base[0 .. m0) or compare(alpha, 0) == 0;
 *   else for an integer structural (jj < n, integer[k][jj] != 0), with fj = alpha - floor(alpha),
 *   g = (fj <= f0) ? fj : rho * (1.0 - fj); else (a continuous structural, or any slack: no integrality of
 *   A or b is assumed) g = (alpha > 0) ? alpha : rho * (-alpha).  Row r reads x_v + sum alpha_jj v_jj = t0
 *   with every v >= 0, so sum g_jj v_jj >= f0 holds at every point whose integer variables are integral,
 *   and the kept optimum (every v_jj = 0) violates it by f0.
 *   the caller's variables -- the stored slack columns are the caller's slacks s_i = b_i - A_i x, so
 *   cut_A[k][t][j] starts at -g_j and takes acc = fma(g_{n+i}, A[i][j], acc) for i = 0 .. m0-1 in that
 *   order, and cut_b[k][t] starts at -f0 and takes acc = fma(g_{n+i}, b[i], acc) in the same order: the row
 *   cut_A x <= cut_b.  (The negation of +0.0 is -0.0; signed zeros are part of the result.)
 *   then -- simplex_solve_batch_device_rows(args', in, out, q) on the explicit grown problem whose rows
 *   m0 .. m are the emitted ones: status, pivots, opt, x, base, objrow, row_width and the out-state are that
 *   call's bit for bit, and so are its warm and cold decisions.  A cold problem's cuts are null rows.
 * The out-state is a state of every state entry and of this one for the shape (n, m), so rounds chain: a
 * later cut whose source row has an earlier cut's slack nonbasic has a non-zero g on it, and substitutes it
 * through that cut's row, a row of A by then.
 * Returns, decided before any device is touched and in this order: -1 args NULL or count < 0; -3 a shape
 * (n, m) of class 0, cuts < 1, cuts >= m, or away not in (0, 0.5] (a NaN is not); 0 for count == 0; -2 cut
 * NULL, integer, cut_A, cut_b or cut_row NULL, a required output NULL, in NULL or incomplete, out incomplete
 * or sharing a member pointer with in, A, b or c NULL; -4 a zero stride of A, b or c along a dimension
 * longer than 1 (the row dimension has length m0), a zero stride of cut_A or cut_b along a dimension longer
 * than 1, a zero integer_sj with n > 1; -5 the workspace, simplex_batch_device_workspace(n, m, count).  The
 * call only enqueues two small memsets and one launch on `stream`. */
typedef struct {
    int cuts;                        /* q >= 1 */
    double away;                     /* in (0, 0.5]: a source row needs away <= frac <= 1 - away */
    const unsigned char *integer;    /* [count][n] through (integer_sb, integer_sj); non-zero: integer variable.
                                        integer_sb may be 0: one mask for every problem */
    long long integer_sb, integer_sj;
    const int *row;                  /* [count][q] dense, or NULL: the kernel chooses */
    double *cut_A;                   /* out [count][q][n] through (cut_A_sb, cut_A_sr, cut_A_sc) */
    long long cut_A_sb, cut_A_sr, cut_A_sc;
    double *cut_b;                   /* out [count][q] through (cut_b_sb, cut_b_si) */
    long long cut_b_sb, cut_b_si;
    int *cut_row;                    /* out [count][q] dense: the source row, -1 for the null row */
} simplex_batch_cut_t;

int simplex_solve_batch_device_cut(const simplex_batch_device_t *args, const simplex_batch_state_t *in,
                                   const simplex_batch_state_t *out /* NULL: not kept */,
                                   const simplex_batch_cut_t *cut);

/* ---- one large LP from device arrays: the engine solve without a host copy of A ---- */
/* twoPhaseMethodEx of one problem held in device memory: A, b and c are read in place through
 * element strides (a transposed or sliced view is not copied; negative strides are accepted, with
 * A, b and c the addresses of the logical first elements), each shard builds its rows of the
 * phase-1 tableau straight from them, and the results are left on the device.  No host copy and no
 * second device copy of A is made (copies of O(m + n) are); one 4-byte read-back decides slack
 * compaction by twoPhaseMethodEx's rule (no b[i] < 0.0).  Every shard setting is honoured as in
 * twoPhaseMethodEx (virtual ranks, a SIMPLEX_GPUS / simplex_set_gpus list, RCCL ranks each holding
 * the whole problem; blocked / row-major storage, regions, alias, compaction, deactivation).
 * A, b and c must lie on the engine's primary device -- the current device (simplex_set_device), or
 * the first of the device list -- whose peers read them through peer access; so must the outputs.
 * Result: twoPhaseMethodEx's for the same values, bit for bit -- *status_out (engine-only statuses
 * included), pivots_out[2], base[m]; *opt_out and x[n] as simplex_solve_batch_device writes them (the
 * objective and getSolutionHost when FEASIBLE, else a quiet NaN and all +0.0, never stale memory);
 * objrow is what simplex_last_objective_row reports: *row_width_out entries (1+n+m after phase 2,
 * 1+n+2m when phase 1 ended the solve, a pivot cap included), +0.0 from there up to 1+n+2m.
 * simplex_last_objective_row, simplex_last_phase_seconds, the TIMER CSV and the verbose lines are
 * twoPhaseMethodEx's.  opt_out and row_width_out may be NULL.
 * The call is synchronous: it waits for `stream` on the host before reading the inputs and returns
 * after all engine work has finished, so the outputs may be used on any stream.  The inputs are
 * not written; the outputs must not overlap them or each other (not checked). */
typedef struct {
    int n, m;                               /* n variables x m constraints, any shape with n >= 1, m >= 1 */
    const double *A; long long A_sr, A_sc;  /* device; element strides: row (constraint), column (variable) */
    const double *b; long long b_si;
    const double *c; long long c_sj;
    long long max_pivots;                   /* as twoPhaseMethodEx */
    double *x;        /* device [n]       or NULL */
    int *base;        /* device [m]       or NULL */
    double *objrow;   /* device [1+n+2m]  or NULL */
    void *stream;     /* hipStream_t the inputs were produced on; NULL = the null stream */
} simplex_device_solve_t;

/* returns 0, -1 args, status_out or pivots_out NULL, -3 n < 1 or m < 1, -2 A, b or c NULL, -4 a
 * stride of 0 on a dimension longer than 1 (all decided before any device is touched), -6 A, b or
 * c not in device memory of the engine's primary device (hipPointerGetAttributes) */
int simplex_solve_device(const simplex_device_solve_t *args, int *status_out, double *opt_out,
                         long long *pivots_out /*[2]*/, int *row_width_out);

/* problem_t from caller arrays (copied; A column-major m x n); free with freeProblem()
 * and then free() of the struct, as the reference's callers do. */
problem_t *simplex_problem_from_arrays(int n, int m, const double *A_colmajor, const double *b,
                                       const double *c);
/* the generator with an explicit CRT flavour: 0 = MSVC rand() (default, matches the
 * published pivot counts), 1 = glibc rand() */
problem_t *simplex_generate_problem_ex(int n, int m, unsigned int seed, int lo, int hi, int rand_kind);
void simplex_free_problem_struct(problem_t *problem);
/* generateRandomProblem computed on the GPU (jump-ahead XORWOW, one thread per row chunk, as
 * the reference's generator.cu does on its GPU); bit-identical to the host generator */
problem_t *simplex_generate_problem_device(int n, int m, unsigned int seed, int lo, int hi, int rand_kind);

/* ---- benchmark session: a resident phase-1 tableau and timed pivots ---- */
typedef struct {
    double wall_ms;            /* device time of the whole call (events on the engine stream) */
    double update_ms;          /* sum of the timed sweep kernel durations (HIP events) */
    long long pivots;          /* pivots applied during the call */
    long long update_launches; /* sweeps timed (those that applied at least one pivot) */
    int status;                /* phase status after the call (SIMPLEX_NOT_ENDED while running) */
    int width;                 /* tableau width N of the phase (reference counting) */
    int stored_width;          /* columns stored (artificials alias slacks in phase 1); a sweep moves all
                                * of them, or 1+n+(touched slacks) under slack compaction */
    long long local_rows;      /* constraint rows owned by this process */
    double update_bytes;       /* bytes per sweep: 16 * local_rows * swept width (read + write of T),
                                * the mean over the timed sweeps */
    long long swept_pivots;    /* timed sweeps: pivots they applied */
    double swept_bytes;        /* timed sweeps: bytes they moved */
} simplex_timing_t;

typedef struct simplex_session simplex_session;
simplex_session *simplex_session_open(problem_t *problem); /* builds phase 1 + canonicalises d */
/* same tableau as simplex_session_open(generateRandomProblem(n, m, seed, lo, hi)), synthesised
 * directly in HBM (each shard generates only its rows; no host copy of A) */
simplex_session *simplex_session_open_generated(int n, int m, unsigned int seed, int lo, int hi, int rand_kind);
/* k pivots (the call ends with a sweep, so the tableau is materialised on return);
 * time_updates = s > 0 brackets every s-th sweep with HIP events */
int simplex_session_pivots(simplex_session *s, long long k, int time_updates, simplex_timing_t *out);
double simplex_session_objective(simplex_session *s);   /* d[0] */
/* the resident tableau in logical column order (m rows of the phase's width at stride ld; T
 * null: not copied), the objective row d and the basis; returns the width, or -1 when rows live
 * on other ranks or the buffer is too narrow */
long long simplex_session_tableau(simplex_session *s, double *T, long long ld, double *d, int *base);
/* slack columns the sweeps currently move (m without slack compaction) */
long long simplex_session_active_slacks(simplex_session *s);
/* the same per shard of this process: returns the number of shards and copies the first `cap`
 * shards' swept slack counts to out (equal on every shard: the permutation is replicated) */
int simplex_session_shard_active_slacks(simplex_session *s, long long *out, int cap);
long long simplex_session_total_pivots(simplex_session *s);
/* pivots per batch (and per sweep) of simplex_session_pivots on this session */
int simplex_session_batch(simplex_session *s);
/* per timed sweep of the last simplex_session_pivots call: pivots it applied and its
 * duration in microseconds; returns the number of sweeps logged (at most cap are copied) */
long long simplex_session_launch_log(simplex_session *s, long long *rows, double *update_us, long long cap);
/* diagnostic: one fused batch of k pivots with in-kernel timestamps (100 MHz ticks) at the
 * hand-off points, out[k][8]: 0 ratio block 0 starts the pivot, 2 its ratios computed, 1 its
 * tile published, 3 objective block 0 knows the selection, 6 it has the leaving row's details,
 * 7 its pivot-row values, 4 its tile published, 5 ratio block 0 knows the next entering
 * variable; -1 when the fused path is not in use */
int simplex_session_stamps(simplex_session *s, int k, unsigned long long *out);
/* the same with every block's own stamps, blk[k][blocks][4] (ratio blocks first: starts the pivot,
 * tile published, knows the next entering variable; objective blocks: knows the selection, has
 * the details, tile published), copied when cap >= k * blocks * 4; returns the blocks (-1 as above) */
int simplex_session_block_stamps(simplex_session *s, int k, unsigned long long *out, unsigned long long *blk,
                                 long long cap);
void simplex_session_close(simplex_session *s);

/* ---- multi-process peer-memory test mode (no RCCL; e.g. 2 processes on one GPU) ----
 * Each process owns rank `rank` of `world` row-block shards (512-aligned blocks, as
 * simplex_dist_init would make them) of a phase-1 state given in logical columns: T_rows =
 * this rank's rows (ld_host doubles apart, width 1+n+2m), d and base whole.  The session's
 * six peer-visible buffers are exported as IPC handles (simplex_ipc_handles_size() bytes);
 * the caller gathers every rank's handles (rank order) and connects; simplex_session_pivots
 * then runs fused multi-rank batches whose hand-offs cross the processes through those
 * mappings.  Returns NULL / < 0 on failure.  Keep every process alive until all have
 * finished their pivots before closing. */
int simplex_ipc_handles_size(void);
simplex_session *simplex_ipc_session_open(int n, int m, int rank, int world, const double *T_rows, long long ld_host,
                                          const double *d, const int *base, unsigned char *handles_out);
int simplex_ipc_session_connect(simplex_session *s, const unsigned char *all_handles);
/* after every process's pivots: write this rank's slice of the objective row into every peer's
 * (between fused batches each rank keeps only its own slice current); barrier the processes
 * before and after.  Returns 0, or -1 for a session that is not in IPC mode. */
int simplex_session_sync_d(simplex_session *s);
/* this process's rows of the resident tableau (logical columns), d and base; returns rows, -1 for
 * ld_host < N, -2 for an IPC session whose objective row is split after its pivots (call
 * simplex_session_sync_d in every process first) */
long long simplex_session_rows(simplex_session *s, double *T_rows, long long ld_host, double *d, int *base);

/* ---- kernel bench (SURVEY.md §8d config 3') ---- */
/* the sweep kernel (solver.cu:34-46's update, `pivots` pending pivots per pass) on a synthetic
 * rows x cols fp64 matrix drawn like generateRandomProblem's A (seed, values in [lo, hi]) with
 * random pending pivots; `warmup` untimed then `iters` timed sweeps (HIP events); returns the
 * average microseconds per sweep (< 0 on bad arguments), *bytes = 16 * rows * cols */
double simplex_bench_sweep(int rows, int cols, unsigned int seed, int lo, int hi, int pivots, int warmup, int iters,
                           double *bytes);

/* ---- kernel-level parity hooks (host arrays in/out, device compute) ---- */
/* epsilon argmin of v[0..L) with the reference combine tree; returns index (or -1) */
long long simplex_dev_argmin(const double *v, long long L, double *vmin);
/* k full pivots on a caller tableau (row-major m x ld, width N) + d + base; returns the
 * phase status after them (SIMPLEX_NOT_ENDED if still running); *done = pivots applied */
int simplex_dev_pivots(double *T, long long m, long long N, long long ld, double *d, int *base, long long k,
                       long long *done);
/* objective canonicalisation d[j] -= sum_i T[i][j] * d[1+base[i]] on the device */
int simplex_dev_update_objective(const double *T, long long m, long long N, long long ld, const int *base,
                                 double *d);
/* phase-1 tableau as built on the device (row-major m x ld, ld >= 1+n+2m), d and base */
int simplex_dev_build_phase1(problem_t *problem, double *T, long long ld, double *d, int *base);
/* the same from the device generator */
int simplex_dev_build_phase1_generated(int n, int m, unsigned int seed, int lo, int hi, double *T, long long ld,
                                       double *d, int *base);
/* the same from device arrays, as simplex_solve_device builds it (A, b: device memory read through
 * element strides; T, d, base: host); returns 0 or simplex_solve_device's -3, -2, -4, -6 */
int simplex_dev_build_phase1_device(int n, int m, const double *A, long long A_sr, long long A_sc, const double *b,
                                    long long b_si, double *T, long long ld, double *d, int *base);

#ifdef __cplusplus
}
#endif
#endif
