// sx_common.hpp -- shared host/device definitions of the MI355X simplex engine.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>


// Status codes: twoPhaseMethod.h:5-8 (reference), solver.cu:77 (NOT_ENDED), plus two
// engine-only codes that the reference has no equivalent for.
#define SX_FEASIBLE 0
#define SX_INFEASIBLE (-1)
#define SX_UNBOUNDED (-2)
#define SX_DEGENERATE (-3)
#define SX_NOT_ENDED (-10)
#define SX_PIVOT_CAP (-11)     // opt-in pivot budget reached (off in parity mode)
#define SX_NUMERIC_FAIL (-12)  // ratio argmin returned no row although a pivot is eligible
#define SX_BAD_SHAPE (-14)     // ragged device batch: a problem's dimensions lie outside the envelope (-13: SX_HANG)
#define SX_BAD_STATE (-15)     // state entry: a problem's saved state fails the kernel's checks

#define SX_TILE 512     // argmin tile = reference THREADS (reduction.cu:6)
#define SX_EPS 1e-9     // macro.h:28

// One 512-element argmin tile winner, plus "this tile has an entry >= eps" for the
// unbounded test.  16 bytes: moved as raw bytes by the tile allgather.
struct __attribute__((aligned(16))) TilePart {
    double v;
    int idx;
    int elig;
};

// Per-shard pivot state, resident in device memory (never read by the host inside a
// batch of pivots).
struct __attribute__((aligned(16))) DevState {
    int status;            // SX_NOT_ENDED while the phase runs
    int e;                 // entering variable of the current pivot (column e+1)
    int r;                 // leaving row (global) of the current pivot
    int pad0;
    double dmin;           // reduced cost of the entering variable (d[e+1] before the pivot)
    long long pivots;      // pivots selected in this phase
    long long max_pivots;  // < 0: no cap (reference behaviour)
    int e_next;            // entering argmin of the updated objective row (next pivot)
    unsigned ticket;       // arrival counter of the ratio/select hand-off (zero between launches)
    double dmin_next;      // its value
    unsigned ticket_d;     // arrival counter of the objective-row blocks of k_pivot_row
    unsigned batch_tag;    // batch id of the last selected pivot ...
    int batch_count;       // ... and the number of pivots selected in that batch
    int pad1;
};

// TilePart.elig: bit 0 = "some entry >= eps" of the tile (the unbounded test)
#define SX_ELIG(x) ((x) & 1)

// Deferred pivots: at most SX_KMAX pivots between two sweeps of the tableau.  A batch runs in
// stages of SX_HMAX slots (the on-chip history of the fused batch, the hand-off records, the
// per-pivot kernels, the vector sweep and the multi-rank batch hold one stage); the one-shard
// fused batch runs two stages, whose 64 pivots the matrix-core sweep applies at once.
#define SX_KMAX 64
#define SX_HMAX 32
// Position of row i's factor of slot s in F: rows in strips of 16, each strip slot-major
// ([strip][slot][16 rows]).  The matrix-core sweep's A operand for 4 slots of a 16-row strip is
// then 64 consecutive doubles (one coalesced load per 4-slot step), and a batch's per-pivot
// factor column is written 16 consecutive doubles per strip.  F holds round_up(rows, 16) rows.
__host__ __device__ constexpr size_t sx_fidx(long long i, int s) {
    return (size_t)(i >> 4) * (16 * SX_KMAX) + (size_t)s * 16 + (size_t)(i & 15);
}
// Batch ids run 1 .. SX_BATCH_IDS - 1: the fused kernels' granule tags keep 15 bits of the id
// (sx_kernels.hip make_tag).  When the ids wrap, the engine clears every id-tagged word (the
// PM pending-leaving masks and the granule records) first, so no stale tag can match.
#define SX_BATCH_IDS (1u << 15)

// Record of one pending pivot (slot s of the current batch).
struct __attribute__((aligned(16))) PivRec {
    int r;     // leaving row (global)
    int e;     // entering variable
    double p;  // pivot element
};

// Device buffers of the pending pivots of a shard, plus the batch id and slot of the pivot
// being enqueued (kernel arguments).
struct Pending {
    // [SX_KMAX][ld] pivot rows (current leaving-row values, before /p).  INVARIANT every writer keeps
    // (k_pivot_row, k_batch / k_batch_mr objective tiles, k_select_row / the row gathers' remote
    // rows, k_activate / activate_block's column exchanges): U[s][j] is the EXACT current value of
    // row r_s at stored column j < Ns just before slot s -- the reference's bits -- for every stored
    // column the sweep touches.  The sweep's leaving-row fix-up (msweep_fixup) and the ratio tiles'
    // leaving-row shortcut restart a row that left at slot sl from U[sl][j] / p_sl instead of its
    // stored value, so they are correct only under this invariant
    // (tests/test_gpu_parity.py::test_row_leaves_twice_per_stage_compacted).
    double *U;
    double *F;               // row factors -(a_ie / p), F[sx_fidx(i, s)]
    PivRec *recs;            // [SX_KMAX]
    unsigned long long *PM;  // [rows] (batch id << 32) | slots < SX_HMAX where the row left the basis
    unsigned long long *PM2; // [rows] the same for slots SX_HMAX + b (bit b): the second stage
    unsigned batch;          // id of the current batch (never 0)
    int q;                   // slot of the pivot being enqueued (pivots pending before it)
};

// Fused batch kernel (k_batch): its exit counter and abort word, each on its own line.
// (The per-pivot hand-offs are data-tagged granules in two arrays of tile records,
// sx_batch_granules_a/b() 8-byte words each.)
struct BatchChan {
    alignas(128) unsigned exit_cnt;  // blocks that have left the kernel
    alignas(128) unsigned abort_w;   // a wait timed out: every block leaves
    alignas(128) unsigned inject_q;  // test hook: 1 + the slot at which ratio block 0 (of rank 0)
                                     // leaves with the batch aborted (0: off); the last block clears it
};

// Multi-rank fused batch (k_batch_mr): every rank's buffers as seen from this rank (peer
// memory over xGMI, or the other virtual shards on one GPU).
#define SX_MAXW 8
struct PeerView {
    const double *T[SX_MAXW];        // tableaux (read: the leaving row)
    unsigned long long *ga[SX_MAXW]; // ratio-tile records (written)
    unsigned long long *gb[SX_MAXW]; // objective-tile records (written)
    unsigned long long *gdone[SX_MAXW];  // batch-end done granules (written)
    double *U[SX_MAXW];              // pending pivot rows (written)
    const double *F[SX_MAXW];        // pending row factors (read: the leaving row's first stage)
    double *d[SX_MAXW];              // objective rows (written)
};

#define SX_HANG (-13)  // fused batch kernel: a hand-off wait timed out (never expected; the host
                       // restores the batch's start state and re-runs it on the per-pivot path)

// Error convention of the reference (error.cu:5-12): print "<msg> in <file> at line <n>"
// and exit(EXIT_FAILURE).
void sx_handle_error(hipError_t err, const char *file, int line);
#define SX_HIP(call) sx_handle_error((call), __FILE__, __LINE__)
void sx_fatal(const char *msg, const char *file, int line);
#define SX_FATAL(msg) sx_fatal((msg), __FILE__, __LINE__)

// Logical vs stored tableau columns.  In phase 1 every artificial column n+m+k starts equal
// to its slack column n+k (both unit vectors, both negated by the b<0 quirk) and receives
// exactly the same IEEE operations at every pivot, so the two stay bit-identical: only
// Ns = 1+n+m columns are stored and logical column j >= art0 reads stored column j - shift.
//
// Slack compaction: while row k has never been a leaving row, its slack
// column is exactly e_k and every pivot leaves it bit-identical (its pivot-row entry is +0).
// Such columns are kept at the end of the stored slack block and the sweep stops before
// them: stored slack position s0 + perm[k] holds logical slack k, and the first *nact
// positions are the columns that have ever been touched.
struct Cols {
    int N;      // logical columns of the phase (reference width: 1+n+2m or 1+n+m)
    int Ns;     // stored columns
    int art0;   // first aliased logical column, or INT_MAX
    int shift;  // alias distance (m)
    int s0;     // first slack column (1+n)
    const int *perm;  // device: logical slack -> stored slack offset, or null (identity)
    __host__ __device__ __forceinline__ int map(int j) const {
        const int k = j >= art0 ? j - shift : j;
        return (perm && k >= s0) ? s0 + perm[k - s0] : k;
    }
};

// Tableau storage in HBM: two regions.  Region A holds stored columns [0, jB) of
// every row at stride ldA; region B, starting offB doubles later, holds stored columns [jB, Ns)
// at stride ldB.  With slack compaction the swept columns [0, 1 + n + nact) lie in region A while
// nact fits, so the sweep streams dense rows (a row of A is only a little wider than what is
// swept) instead of a prefix of every full-width row; without a region B (jB = Ns, the default for
// small m and for callers' tableaux) there is one region.  jB is a multiple of 512, so no
// 512-column tile straddles the two.
// Inside a region, blk = 0: plain row-major (callers' tableaux: tabular.h); blk = 1 (the engine's
// own tableaux): 16-row strips of ld * 16 doubles, each strip a sequence of 4-column
// groups of 64 doubles, each group 4 blocks of 4 rows x 4 columns (one 128-byte line each).  A
// column of 512 rows then spans 128 lines instead of 512 (the fused batch's entering-column
// gather), a row's 512 columns 128 lines instead of 32 (its pivot-row read), and a strip is still
// one contiguous range (the sweep); two adjacent columns 2c, 2c + 1 of a row stay adjacent.
// Rows are allocated in whole strips.
struct TLay {
    size_t ldA = 0, ldB = 0, offB = 0;
    int jB = 0x7fffffff;
    int blk = 0;
    __host__ __device__ __forceinline__ static size_t b4(long long i, int j, size_t ld) {
        return (size_t)(i >> 4) * 16 * ld + (size_t)(j >> 2) * 64 + (size_t)(((int)i & 15) >> 2) * 16 +
               (size_t)(((int)i & 3) * 4 + (j & 3));
    }
    __host__ __device__ __forceinline__ size_t idx(long long i, int j) const {
        if (blk) return j < jB ? b4(i, j, ldA) : offB + b4(i, j - jB, ldB);
        return j < jB ? (size_t)i * ldA + (size_t)j : offB + (size_t)i * ldB + (size_t)(j - jB);
    }
};

// ---- kernel launchers (sx_kernels.hip) ----
struct SweepCfg {
    int batch;  // pivots per sweep (1..SX_KMAX; the vector sweep: up to SX_HMAX)
    int mfma;   // 1: the matrix-core sweep (k_msweep), 0: the vector sweep (k_sweep)
};

int sx_enter_blocks(int L);
void sx_launch_enter(const double *d, int L, TilePart *parts, DevState *st, hipStream_t s);
void sx_launch_ratio_select(const double *T, int rows, int row0, size_t ld, TLay tl, TilePart *tiles_local, double *colE,
                            DevState *st, int *base, bool select, double *slots, size_t slot_stride, Cols c,
                            const Pending &pd, hipStream_t s);
void sx_launch_select_gathered(const double *slots, size_t slot_stride, int B2, int *base, DevState *st,
                               const Pending &pd, hipStream_t s);
void sx_launch_select_row(const double *T, int rows, int row0, size_t ld, TLay tl, Cols c, const TilePart *tiles_all, int B2,
                          double *prow_out, int *base, DevState *st, const Pending &pd, hipStream_t s);
void sx_launch_pivot_row(const double *T, int rows, int row0, size_t ld, TLay tl, Cols c, double *d, const double *prow_buf,
                         size_t prow_stride, const double *colE, DevState *st, const Pending &pd,
                         TilePart *enter_parts, hipStream_t s);
// nact (device, or null): sweep only the columns [0, s0 + *nact) (slack compaction)
void sx_launch_sweep(double *T, int rows, int row0, size_t ld, TLay tl, int Ns, const int *nact, int s0,
                     const Pending &pd, const DevState *st, int rev, SweepCfg cfg, hipStream_t s);
// slack compaction, after a batch's selections and before its sweep: move the slack column
// of every row that left the basis for the first time into the swept block
// (ucol[r]: the unswept slack column that is the unit vector e_r, or -1; urow[k]: the row of unswept
// slack k's unit vector -- k itself until row k first leaves)
void sx_launch_activate(int *perm, int *iperm, int *ucol, const int *urow, int *nact, int m, double *T, int rows,
                        int row0, size_t ld, TLay tl, int s0, const Pending &pd, const DevState *st, int slots,
                        hipStream_t s);  // slots: the batch size (two passes above SX_HMAX)
// after a sweep (every few batches): the swept slack columns whose slack is basic (exact unit
// vectors, checked) moved behind the swept block (k_deact_*) -- on one shard, or on
// the row-block shards of one process, which plan from their combined verdicts (DeactPeers)
#define SX_DEACT_CAP 4096  // columns per round (a multiple of 1024)
struct DeactList {
    int C;    // listed columns (swept slacks that are basic), stored-position order
    int nsw;  // column exchanges of the round
    int x[SX_DEACT_CAP], r[SX_DEACT_CAP], bad[SX_DEACT_CAP];  // position, unit row, failed the check
    int dst[SX_DEACT_CAP], src[SX_DEACT_CAP], row[SX_DEACT_CAP];
};
// (tag: [m] position tags, zero at allocation; epoch: this round's number, from 1; check: compare each
// column with its unit vector first -- required: an entered column is e_r only where its entries'
// residuals a_k - fl(a_k / p) p round to 0; fail: [m] slack -> 1 + the row it failed the check in, zero
// at allocation)
// peers = false: the whole round on one shard.  peers = true: only the list and this shard's check
// (mark / list / check); once every shard's check has finished, sx_launch_deactivate_apply plans from
// all the shards' verdicts and moves this shard's rows
void sx_launch_deactivate(int *perm, int *iperm, int *ucol, int *urow, int *nact, const int *base, int n, int m,
                          bool alias, double *T, int rows, int row0, TLay tl, int s0, unsigned long long *tag,
                          unsigned epoch, bool check, int *fail, DeactList *L, hipStream_t s, bool peers = false);
// the shards' verdict arrays (DeactList::bad of every shard of the process, rank order; this
// shard's own among them), passed to k_deact_plan by value
struct DeactPeers {
    const int *bad[SX_MAXW];
    int nw;
};
void sx_launch_deactivate_apply(int *perm, int *iperm, int *ucol, int *urow, int *nact, double *T, int rows, int row0,
                                TLay tl, int s0, int *fail, DeactList *L, const DeactPeers &peers, hipStream_t s);
// fused batch of up to k pivots on one shard (ratio tiles + objective tiles in one resident
// grid); returns false (nothing launched) when the grid cannot be resident at once
bool sx_batch_fits(int rows, Cols c, int k);
int sx_batch_obj_tile_limit();  // objective tiles a one-shard fused batch holds (logical width <= 512 x this + 1)
// d_save: the objective row as the batch found it (restored by the host after SX_HANG); the
// basis is written only by a batch that completed
// perm / iperm / ucol / urow / nact (slack compaction, or null): the batch's last block also activates
// the slack columns of the rows that left the basis for the first time (k_activate's work)
void sx_launch_batch(const double *T, int rows, size_t ld, TLay tl, Cols c, double *d, double *d_save, int *base,
                     DevState *st, const Pending &pd, int k, BatchChan *chan, unsigned long long *ga,
                     unsigned long long *gb, unsigned long long *stamps, int *perm, int *iperm, int *ucol,
                     const int *urow, int *nact, int m, hipStream_t s);
size_t sx_batch_granules_a();
size_t sx_batch_granules_b();
// the multi-rank fused batch: `grids` co-resident launches of this shape must fit the device
bool sx_batch_mr_fits(int slots, int nb_local, int k, int grids);
void sx_launch_batch_mr(const double *T, int rows, int row0, int rpr, size_t ld, TLay tl, Cols c, double *d, double *d_save,
                        int *base, DevState *st, const Pending &pd, int k, int slots, int W, int rank, int tb0, int tb1,
                        int repl, BatchChan *chan, const unsigned long long *ga, const unsigned long long *gb,
                        const unsigned long long *gdone, const PeerView &pv, unsigned long long timeout,
                        hipStream_t s);
// one rank of a multi-rank launch
struct MrLaunchRank {
    const double *T;
    int rows, row0, rank, tb0, tb1;
    int repl;  // replicated objective: every rank runs every objective tile (tb0 = 0, tb1 = all)
    const int *perm;
    double *d, *d_save;
    int *base;
    DevState *st;
    Pending pd;
    BatchChan *chan;
    const unsigned long long *ga, *gb, *gdone;
};
// the batches of the nloc ranks (of W) that share one GPU, as one launch
void sx_launch_batch_mr_multi(const MrLaunchRank *ranks, int nloc, int W, int rpr, size_t ld, TLay tl, Cols c, unsigned B,
                              int k, int slots, const PeerView &pv, unsigned long long timeout, hipStream_t s);
void sx_set_update_waves(float w);  // resident-grid multiple of the sweep (default 1)
void sx_set_sweep_record(int *rec);  // next sweeps write (batch tag, count, nact) to rec[0..2] (null: off)
void sx_launch_sum_rows(double *out, const double *const *srcs, int nsrc, int N, hipStream_t s);
void sx_launch_l2_writeback(hipStream_t s);  // every XCD's L2 writes back its dirty lines
// diagnostic: every shard's pending pivot rows of batch B against shard 0's (counts mismatches in *bad)
void sx_launch_check_u(const PeerView &pv, int W, size_t ld, int Ns, const DevState *st, unsigned B,
                       unsigned long long *bad, hipStream_t s);
// a rank's contribution to the objective-row gather: d on [j0, j1) (and d[0] if with0), -0.0 elsewhere
void sx_launch_d_contrib(const double *d, double *out, int N, int j0, int j1, int with0, hipStream_t s);

void sx_launch_coef(const double *d, const int *base, int row0, int rows, double *coef, hipStream_t s);
void sx_launch_gemv_partials(const double *T, int rows, TLay tl, int Ns, const double *coef, double *partials,
                             hipStream_t s);
void sx_launch_gemv_apply(double *d, Cols c, const double *partials, int nblk, hipStream_t s);

// One LP read in place from device memory: A(i, j) = A[i * A_sr + j * A_sc], b_i = b[i * b_si],
// c_j = c[j * c_sj] (element strides).  A column-major m x n array is A_sr = 1, A_sc = m.
struct SxSource {
    const double *A;
    long long A_sr, A_sc;
    const double *b;
    long long b_si;
    const double *c;
    long long c_sj;
};
// the generator path's filler: column 0 = b, the identity columns and the negation of the rows
// with compare(b_i) < 0, around structural columns that are already in T
void sx_launch_fill_generated(double *T, int rows, int row0, TLay tl, int n, int m, int Ns, const double *b_full,
                              hipStream_t s);
// the whole tableau (stored columns [0, Ns) of the shard's rows) in one pass from src.  src.A is the
// address of the SHARD's first row of A; src.b is the whole b (row row0 + i reads b[(row0 + i) * b_si])
void sx_launch_build_strided(double *T, int rows, int row0, TLay tl, int n, int m, int Ns, const SxSource &src,
                             hipStream_t s);
void sx_launch_copy_strided(double *dst, const double *src, long long stride, int count, hipStream_t s);
// *flag (zero at launch) = 1 when some b_i < 0.0
void sx_launch_any_negative(const double *b, long long b_si, int m, int *flag, hipStream_t s);
// dst[0, w) = src[0, w), dst[w, total) = +0.0
void sx_launch_copy_pad(double *dst, const double *src, int w, int total, hipStream_t s);
// x[base[i]] = rhs[i] for base[i] < n (x zero at launch)
void sx_launch_scatter_solution(double *x, int n, const int *base, const double *rhs, int m, hipStream_t s);
void sx_launch_init_vectors(double *d, int N1, int n, int m, int *base, hipStream_t s);
void sx_launch_phase2_costs(double *d, int n, int m, const double *c, hipStream_t s);
void sx_launch_gather_rhs(const double *T, int rows, TLay tl, double *out, hipStream_t s);
// rows [i0, i0 + nr), stored columns [0, Ns) -> row-major out (nr x Ns); and row-major in (pitch
// ld_in) -> stored columns [j0, j0 + Ns) of those rows
void sx_launch_rows_out(const double *T, TLay tl, int i0, int nr, int Ns, double *out, hipStream_t s);
void sx_launch_rows_in(double *T, TLay tl, int i0, int nr, int Ns, int j0, const double *in, size_t ld_in,
                       hipStream_t s);
// device generator (sx_generator.hip) and the CRT seeding (sx_problem.cpp)
void sx_crt_seeds(unsigned seed, int kind, uint32_t out[3]);
void sx_launch_gen_rows(uint32_t seedA, int n, int m, int row0, int rows, double lo, double hi, double *T, TLay tl,
                        double *A_cm, hipStream_t s);
void sx_launch_gen_vector(uint32_t seed, long long first, int count, double lo, double hi, double *out,
                          hipStream_t s);

void sx_launch_argmin_vector(const double *v, long long L, TilePart *parts, int *out_idx, double *out_v,
                             hipStream_t s);

// ---- batched solve: one workgroup carries one whole LP (sx_batch.hip) ----
// Dynamic LDS a resident workgroup may claim: the CU's 160 KiB less 512 bytes for the kernel's
// static reduction scratch.  A problem whose working set fits is LDS-resident (class 2).
#define SX_BATCH_LDS_BYTES (160 * 1024 - 512)
// Workspace-resident cap (class 1): a working set of at most this many doubles (4 MiB) in a
// per-workgroup slice of device memory; larger problems go to the engine (class 0).
#define SX_BATCH_WS_DOUBLES (1 << 19)
// ... and all the slices of one launch together take at most this many bytes
#define SX_BATCH_WS_BYTES (1ull << 30)
// Default resident pivot budget per phase (simplex_set_batch_budget(0)); ordinary small instances
// need n + m to 2 (n + m) pivots.
__host__ __device__ constexpr long long sx_batch_default_budget(int n, int m) {
    return 64 + 16 * ((long long)n + (long long)m);
}

// Working set of one resident problem, in doubles from its start: T (m rows of the 1 + n + m stored
// columns at an odd stride ld), d at the full phase-1 width 1 + n + 2m, the pivot-row copy, colE,
// the argmin tile winners and the basis.  Every offset is even (TilePart is 16-byte aligned).
struct BatchLay {
    int ld;
    long long d, prow, colE, parts, base, total;
};
__host__ __device__ constexpr long long sx_even(long long x) { return (x + 1) & ~1LL; }
__host__ __device__ constexpr BatchLay sx_batch_lay(int n, int m) {
    const long long Ns = 1 + (long long)n + m, N1 = Ns + m;
    const long long ld = Ns | 1;
    const long long L = (N1 - 1 > m ? N1 - 1 : m), tiles = (L + SX_TILE - 1) / SX_TILE;
    BatchLay l{};
    l.ld = (int)ld;
    l.d = sx_even(ld * m);
    l.prow = l.d + sx_even(N1);
    l.colE = l.prow + sx_even(Ns);
    l.parts = l.colE + sx_even(m);
    l.base = l.parts + 2 * tiles;
    l.total = l.base + sx_even((m + 1) / 2);
    return l;
}
// 2 LDS-resident, 1 workspace-resident, 0 engine (also every shape without a variable or a constraint)
__host__ __device__ constexpr int sx_batch_class(int n, int m) {
    if (n < 1 || m < 1) return 0;
    const long long t = sx_batch_lay(n, m).total;
    return t * 8 <= SX_BATCH_LDS_BYTES ? 2 : t <= SX_BATCH_WS_DOUBLES ? 1 : 0;
}

// One resident problem of a batch call: its shape and where its input (A column-major, b, c) and
// its output (the final RHS column, then the basis as ints) lie, in doubles from the buffers' starts.
struct __attribute__((aligned(16))) BatchProb {
    int n, m;
    long long in_off, out_off;
    long long pad;
};
struct __attribute__((aligned(16))) BatchRes {
    double opt;
    long long p1, p2;
    int status;
    int evicted;  // 1: the resident budget ran out; the host re-solves the problem on the engine
};
struct BatchArgs {
    const BatchProb *probs;
    const int *order;   // [count] problems of this launch, larger first
    int count;
    unsigned *counter;  // the launch's work counter (zero at launch)
    const double *in;
    BatchRes *res;
    double *out;
    double *ws;         // workspace-resident: the slices; null for the LDS class
    long long slice;    // doubles per slice
    long long max_pivots;  // per phase, < 0: none (status SX_PIVOT_CAP)
    long long budget;      // resident pivots per phase, 0: sx_batch_default_budget
};
// The device-resident entry (simplex_solve_batch_device): `count` problems of one shape read in
// place from strided device arrays (element strides: batch, constraint row, variable column), every
// result written to dense device arrays by the kernel's epilogue.  Problem k of the launch is the
// work counter's value; there are no per-problem records.  The fields' order is part of the kernel's
// speed: with the strided source grouped in front of the batch strides k_batch_solve_dev measured 3 %
// slower at 64x64, so the source stays spelled out in the caller's order.
struct BatchDevArgs {
    int n, m, count;
    const double *A;
    long long A_sb, A_sr, A_sc;
    const double *b;
    long long b_sb, b_si;
    const double *c;
    long long c_sb, c_sj;
    long long max_pivots;  // per phase, < 0: none (status SX_PIVOT_CAP)
    long long budget;      // resident pivots per phase, 0: sx_batch_default_budget
    int *status;           // [count]; an evicted problem gets SX_NOT_ENDED
    long long *pivots;     // [count][2]
    double *opt;           // [count]: d[0] when FEASIBLE, else a quiet NaN
    double *x;             // [count][n] or null: getSolutionHost when FEASIBLE, else +0.0
    int *base;             // [count][m] or null
    double *objrow;        // [count][1 + n + 2m] or null: the final objective row, zero-padded
    int *row_width;        // [count] or null: 1 + n + m after phase 2, 1 + n + 2m after phase 1, 0 evicted
    int *evicted;          // [1] problems left SX_NOT_ENDED (zero at launch)
    unsigned *counter;     // the launch's work counter (zero at launch)
    double *ws;            // workspace-resident: the slices; null for the LDS class
    long long slice;       // doubles per slice
};
// The ragged device entry (simplex_solve_batch_device_ragged): BatchDevArgs, whose n and m are now
// the envelope every input and output array is shaped by, plus the per-problem dimensions.  Problem
// k is the n_k[k] x m_k[k] leading block of its envelope slot; nothing outside that block is read.
struct BatchRagArgs : BatchDevArgs {
    const int *n_k, *m_k;  // [count] device; out of [1, n] / [1, m]: the problem gets SX_BAD_SHAPE
    const int *order;      // [count] device or null (identity): the work counter's value -> problem
    long long set;         // doubles of the envelope's working set, sx_batch_lay(n, m).total
};
// The state entry (simplex_solve_batch_device_state): BatchDevArgs plus the saved states it loads
// and writes.  A state is dense per problem: T [m][1 + n + m] (the stored columns b | structural |
// slack), d [1 + n + 2m], base [m], phase (1, 2; 3 for the right-hand-side entry alone; 0: none) and
// pivots [2].
struct BatchState {
    double *T, *d;
    int *base, *phase;
    long long *pivots;
};
struct BatchStArgs : BatchDevArgs {
    BatchState in;   // T null: a fresh solve from A, b, c; else only c is read
    BatchState out;  // T null: the state is not kept; may equal `in` member for member
    int recost;      // a phase-2 state restarts phase 2 on the call's costs
};
// The right-hand-side entry (simplex_solve_batch_device_rhs): the state entry's arguments with `in`
// required; a state's phase may also be 3, phase 2's tableau inside the dual loop.
struct BatchRhsArgs : BatchDevArgs {
    BatchState in;   // required
    BatchState out;  // T null: the state is not kept; may equal `in` member for member
    int rerhs;       // b is a new right-hand side for the kept states; 0: a resume, only c is read
};
// The rows entry (simplex_solve_batch_device_rows): n and m are the grown shape; `in` has the shape
// (n, m - added) and `out` the grown one, so the two never coincide.
struct BatchRowsArgs : BatchDevArgs {
    BatchState in;   // required; dense at the in-state's own strides
    BatchState out;  // T null: the state is not kept
    int added;       // constraint rows appended behind the in-state's, in [1, m)
};
// The columns entry (simplex_solve_batch_device_cols): n and m are the grown shape; `in` has the shape
// (n - added, m) and `out` the grown one, so the two never coincide.
struct BatchColsArgs : BatchDevArgs {
    BatchState in;   // required; dense at the in-state's own strides
    BatchState out;  // T null: the state is not kept
    int added;       // structural columns appended behind the in-state's, in [1, n)
};
// The drop entry (simplex_solve_batch_device_drop): n and m are the reduced shape; `in` has the shape
// (n, m + dropped) (kind 0) or (n + dropped, m) (kind 1) and `out` the reduced one, so the two never
// coincide.  The working set, ws and slice are the in-state's shape's.
struct BatchDropArgs : BatchDevArgs {
    BatchState in;    // required; dense at the in-state's own strides
    BatchState out;   // T null: the state is not kept
    int kind;         // 0: constraint rows, 1: structural columns
    int dropped;      // q >= 1 indices per problem
    const int *idx;   // [count][dropped] device: strictly ascending, in [0, m + q) or [0, n + q)
};
// The branch entry (simplex_solve_batch_device_branch): n, m and count are the children's; A, b and c
// hold `roots` problems of m - depth rows, `in` holds `parents` problems of shape (n, m - 1) and `out`
// count problems of the children's shape.  Child k continues in-state problem parent[k] on the problem
// root[k], whose rows are followed by the bound rows coef[k][t] x_var[k][t] <= rhs[k][t], t < depth; the
// last of them is the new one.
struct BatchBranchArgs : BatchDevArgs {
    BatchState in;    // required; dense at the in-state's own strides, indexed by parent[k]
    BatchState out;   // T null: the state is not kept
    int roots, parents;
    int depth;        // q in [1, m): bound rows per child
    const int *root, *parent;  // [count] device: outside [0, roots) / [0, parents) the child gets SX_BAD_STATE
    const int *var;            // [count][depth] device, dense: outside [0, n) the child gets SX_BAD_STATE
    const double *coef, *rhs;  // [count][depth] device, dense
};
// The cut entry (simplex_solve_batch_device_cut): the rows entry's shapes -- n and m are the grown shape,
// `in` has the shape (n, m - cuts) -- but the new rows are outputs: A and b hold the m - cuts rows the
// in-state was solved with, and the kernel writes the cuts it derives to cut_A and cut_b, which may be
// rows m - cuts .. m of the same arrays.
struct BatchCutArgs : BatchDevArgs {
    BatchState in;   // required; dense at the in-state's own strides
    BatchState out;  // T null: the state is not kept
    int cuts;        // q in [1, m): cuts per problem
    double away;     // a source row's fractional part lies in [away, 1 - away]
    const unsigned char *integer;  // [count][n] through the strides; non-zero: an integer variable
    long long integer_sb, integer_sj;
    const int *row;  // [count][cuts] dense, or null: the kernel chooses the source rows
    double *cut_A;   // out [count][cuts][n]
    long long cut_A_sb, cut_A_sr, cut_A_sc;
    double *cut_b;   // out [count][cuts]
    long long cut_b_sb, cut_b_si;
    int *cut_row;    // out [count][cuts] dense: the source row, -1 for the null row
};
// Bytes in front of the slices in a caller's workspace: the work counter, on a line of its own.
#define SX_BATCH_DEV_HEADER 256

// The ten entries of sx_batch.hip, one kernel pair (LDS, workspace) each.
enum class BatchEntry { Host, Dev, Rag, St, Rhs, Rows, Cols, Drop, Branch, Cut };
// workgroups of that entry's kernel the current device holds at once with this much dynamic LDS
int sx_batch_resident(BatchEntry entry, bool lds, size_t lds_bytes);
// one launch of the entry the argument struct belongs to
void sx_launch_batch_solve(bool lds, const BatchArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchDevArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchRagArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchStArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchRhsArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchRowsArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchColsArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchDropArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchBranchArgs &a, int grid, size_t lds_bytes, hipStream_t s);
void sx_launch_batch_solve(bool lds, const BatchCutArgs &a, int grid, size_t lds_bytes, hipStream_t s);
