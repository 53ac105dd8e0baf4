/*
 * lpgpu.h -- C-ABI of the MI355X dense simplex pivot engine (liblpgpu.so).
 *
 * The reference (tkoz0/linear-program-solver, package lpsol) is pure Python
 * with no FFI: its "operator API" for the hot path is the method surface
 * Simplex calls on Tableau.  Per-element getters cannot
 * cross a device boundary cheaply, so the boundary is lifted one level: each
 * entry point below replaces a whole reference method (cited file:line), and
 * the Python front-end (linear-program-solver_amd/lpsol_amd) binds them with
 * ctypes behind the reference's own class and method names.
 *
 * Conventions
 *   - The tableau is (m+1) x (n+1) float64, row-major.  Row 0 is
 *     [_z, c_0..c_{n-1}] with _z the stored NEGATED objective
 *     (lpsol/tableau.py:46,82-84); row 1+i is [b_i, a_i0..a_i,n-1].
 *   - r indexes constraints (0..m-1), c indexes variables (0..n-1), exactly
 *     like the reference's pivot(r, c).
 *   - Host buffers are caller-owned and copied synchronously.  The library
 *     owns all device memory.  A handle is used by one host thread at a time.
 *   - No exceptions cross the ABI: every call returns an lp_status; the
 *     front-end maps them to the reference's exceptions.
 */
#ifndef LPGPU_H
#define LPGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum lp_status {
    LP_PIVOTED = 0,      /* a pivot was found (and performed, where asked)   */
    LP_OPTIMAL = 1,      /* 'optimal'   simplex.py:233-234,268-269            */
    LP_UNBOUNDED = 2,    /* 'unbounded' simplex.py:245-246,280-281            */
    LP_ZERO_PIVOT = -1,  /* ZeroDivisionError('zero pivot r,c') tableau.py:300-301 */
    LP_BAD_ARG = -2,     /* ValueError / IndexError in the reference          */
    LP_DEVICE_ERROR = -3,/* HIP or RCCL failure; see lp_last_error            */
    LP_CAP_REACHED = -4, /* extension: pivot cap hit before optimality        */
    LP_BAD_PIVOT = -5,   /* ValueError('bad pivot by min ratio test') simplex.py:214-215 */
    LP_OBJ_INCREASED = -6,/* AssertionError('objective value increased') simplex.py:133:
                            a standard-rule pivot of lp_solve left the objective above
                            its value at the start of the call by more than the stall
                            tolerance; the solve stops after that pivot */
    LP_INFEASIBLE = -7,  /* ValueError('infeasible problem') simplex.py:64-67 (lp_twophase_solve) */
    LP_PHASE1_FAILED = -8 /* the reference's phase-1 internal-error assertions
                            simplex.py:63,73 (lp_twophase_solve) */
} lp_status;

typedef enum lp_rule {
    LP_RULE_STANDARD = 0,  /* findPivotStandard   simplex.py:251-284 */
    LP_RULE_MIN_INDEX = 1, /* findPivotMinIndex   simplex.py:218-249 */
    LP_RULE_MAX_INCREASE = 2, /* findPivotMaxIncrease simplex.py:286-328; lp_batch_run only
                                (lp_run and lp_find_pivot refuse it: the single-LP engine
                                has lp_find_pivot_max_increase) */
    LP_RULE_DUAL = 3       /* one dual simplex step (the reference has none); lp_batch_run
                              only, see there */
} lp_rule;

/* Float64 stand-ins for the reference's exact rational comparisons. */
typedef struct lp_tol {
    double cost;      /* c_j is negative iff c_j < -cost     (simplex.py:229,264)  */
    double cost_tie;  /* standard rule: first j with c_j <= g + cost_tie*|g|,
                         g = min c_j                        (simplex.py:266)       */
    double pivot;     /* a_ij is positive iff a_ij > pivot  (simplex.py:239,274)  */
    double zero;      /* |b_i| <= zero counts as b_i = 0 in the ratio             */
    double ratio_tie; /* first i with q_i <= g + ratio_tie*|g| (simplex.py:242,277) */
    double stall;     /* |z - z0| <= stall*max(1,|z0|) is "unchanged" (simplex.py:134) */
} lp_tol;

typedef struct lp_handle lp_handle;

/* Defaults: cost 1e-9, cost_tie 1e-12, pivot 1e-9, zero 1e-9, ratio_tie 1e-12,
 * stall 1e-12. */
void lp_default_tol(lp_tol *tol);

/* Number of visible GPUs. */
int lp_device_count(int *count);

/* Tableau(m, n) on one GPU (lpsol/tableau.py:36-52): allocates a zeroed
 * (m+1) x ld device tableau, ld = n+1 rounded up to 64 doubles.
 * m <= 0 or n <= 0 -> LP_BAD_ARG (the reference raises ValueError, :40-43). */
int lp_create(int64_t m, int64_t n, int device, lp_handle **out);

/* Row-sharded tableau for one rank of an nranks-process job (one GPU per
 * process).  Constraint rows are split in contiguous blocks; row 0 (the
 * objective) is replicated on every rank.  uid is the 128-byte RCCL unique id
 * from lp_comm_unique_id on rank 0, broadcast to all ranks by the caller;
 * uid NULL creates no RCCL communicator (the device-side peer exchange below
 * must then be set up, or the host's all-gather given with
 * lp_set_host_allgather, for the per-pivot exchanges). */
int lp_comm_unique_id(void *uid128);
int lp_create_sharded(int64_t m, int64_t n, int device, int rank, int nranks,
                      const void *uid128, lp_handle **out);
/* In-process emulation of an nshards-rank job on ONE device: nshards handles
 * (written to out[0..nshards-1]) that share a stream and exchange through
 * device copies instead of RCCL.  Driving any member (lp_solve, lp_run,
 * lp_find_pivot, lp_pivot, ...) drives all of them in lock-step.  Used by the
 * test-suite to prove the pivot sequence is independent of the shard count. */
int lp_create_group(int64_t m, int64_t n, int device, int nshards, lp_handle **out);
/* This rank's constraint-row block [*row_begin, *row_begin + *row_count). */
int lp_shard_rows(const lp_handle *h, int64_t *row_begin, int64_t *row_count);

/* Device-side exchange between the ranks of a sharded job (one GPU per
 * rank): the pivot selection runs as one persistent kernel per rank and
 * group of pivots, exchanging the leaving-row candidates and the pivot row
 * through the ranks' exchange buffers (peer stores over xGMI) instead of one
 * RCCL collective per pivot.  Setup is collective:
 *   lp_peer_handle  -> this rank's exchange-buffer IPC handle (LP_PEER_HANDLE_BYTES)
 *   (the caller all-gathers the handles in rank order)
 *   lp_peer_open    -> opens the peers' buffers and checks the exchange with
 *                      a ping between all ranks; LP_DEVICE_ERROR if it fails
 * If any rank fails, every rank calls lp_peer_enable(h, 0): the RCCL
 * per-pivot path stays in use (identical results).  In-process shard groups
 * (lp_create_group) set this up themselves. */
#define LP_PEER_HANDLE_BYTES 64
int lp_peer_handle(lp_handle *h, void *handle);
int lp_peer_open(lp_handle *h, const void *handles);
int lp_peer_enable(lp_handle *h, int enable);

/* The host's own all-gather for a multi-process sharded handle (gloo, MPI,
 * ...): fn(ctx, send, recv, bytes) must gather `bytes` from every rank into
 * recv in rank order (nranks * bytes) and return 0.  It combines the column
 * scans' per-column results (lp_find_pivot_max_increase, lp_find_pivot_all,
 * lp_form_checks; RCCL is used when this is not set) and, on a handle
 * created without an RCCL communicator, carries the per-pivot exchanges of
 * the per-pivot path (explicit and validated pivots, peer exchange disabled)
 * synchronously.  No reference counterpart (the reference is one process);
 * it replaces the collective the scans of simplex.py:286-360 and
 * tableau.py:466-521 need once the rows are split across processes.
 * LP_BAD_ARG on a handle that is not a multi-process shard. */
typedef int (*lp_allgather_fn)(void *ctx, const void *send, void *recv, int64_t bytes);
int lp_set_host_allgather(lp_handle *h, lp_allgather_fn fn, void *ctx);

int lp_destroy(lp_handle *h);

int lp_set_tol(lp_handle *h, const lp_tol *tol);
int lp_get_tol(const lp_handle *h, lp_tol *tol);

/* Bulk copies of tableau rows [row0, row0+nrows) (row 0 = objective) to and
 * from a host row-major buffer with leading dimension ldh >= n+1.  Replace the
 * reference's setZ/setC/setB/setA (tableau.py:128-158) and getZ/getC/getB/getA
 * (tableau.py:82-108).  On a sharded handle the rows are GLOBAL indices and
 * must be row 0 or lie inside this rank's block.  A window that is refused
 * (LP_BAD_ARG) is refused as a whole: no row of it is copied. */
int lp_upload_rows(lp_handle *h, int64_t row0, int64_t nrows, const double *src, int64_t ldh);
int lp_download_rows(lp_handle *h, int64_t row0, int64_t nrows, double *dst, int64_t ldh);

/* Tableau.pivot(r, c) (tableau.py:295-308).  a_rc == 0 -> LP_ZERO_PIVOT and
 * the tableau is untouched. */
int lp_pivot(lp_handle *h, int64_t r, int64_t c);

/* findPivotStandard / findPivotMinIndex (simplex.py:218-284): selects (r, c)
 * by rule and, if do_pivot, performs it.  Returns LP_PIVOTED (found),
 * LP_OPTIMAL or LP_UNBOUNDED. */
int lp_find_pivot(lp_handle *h, int rule, int do_pivot, int64_t *r, int64_t *c);

/* Simplex.pivot(r, c) (simplex.py:199-216): pivot only if row r attains the
 * minimum ratio in column c, else LP_BAD_PIVOT and nothing changes. */
int lp_pivot_checked(lp_handle *h, int64_t r, int64_t c);

/* Simplex.solve (simplex.py:110-148) entirely on the device: standard-rule
 * pivots until the stall counter (pivots leaving the objective equal to its
 * value at the start of the call) reaches m+n, then min-index pivots to
 * optimality.  max_pivots < 0 means no cap.  Returns LP_OPTIMAL, LP_UNBOUNDED
 * (the reference raises AssertionError there) or LP_CAP_REACHED.
 * *npiv = pivots done, *nstd = of which standard-rule. */
int lp_solve(lp_handle *h, int64_t max_pivots, int64_t *npiv, int64_t *nstd);

/* k pivots of one rule with no stall logic (the fixed-K benchmark loop, i.e.
 * findPivot*(do_pivot=True) called k times).  Stops early on optimal or
 * unbounded.  Returns the last status; *done = pivots performed.  k = 0 is
 * LP_PIVOTED with *done = 0 and an empty pivot log, whatever the tableau. */
int lp_run(lp_handle *h, int rule, int64_t k, int64_t *done);

/* findPivotMaxIncrease (simplex.py:286-328): over columns with c_j < -cost,
 * the largest objective increase -c_j * (min ratio of column j); ties to the
 * first column, its ratio-test row.  LP_UNBOUNDED if any such column has no
 * eligible row (the reference returns at the first one, :319-320),
 * LP_OPTIMAL if no column qualifies; performs the pivot if do_pivot.  On a
 * multi-process sharded handle every rank calls it (collective: the ranks'
 * per-column results are all-gathered, see lp_set_host_allgather). */
int lp_find_pivot_max_increase(lp_handle *h, int do_pivot, int64_t *r, int64_t *c);

/* findPivotAll (simplex.py:330-360): every min-ratio pivot of every column,
 * column-major, rows in order; writes up to cap (r, c) pairs, *count = all.
 * Collective on a multi-process sharded handle (every rank gets all pairs). */
int lp_find_pivot_all(lp_handle *h, int64_t *rc, int64_t cap, int64_t *count);

/* Form checks of the current tableau, exact comparisons of the float64 values
 * (tableau.py:466-521): flags[0] isCanonical, [1] isOptimal, [2] isUnbounded,
 * [3] isInfeasible, [4] isDegenerate.  bcols (m entries, may be NULL) gets
 * isCanonical's basic column per row (-1: none) unless some b_i < 0, where
 * the reference leaves it untouched.  Collective on a multi-process sharded
 * handle. */
int lp_form_checks(lp_handle *h, int32_t *flags, int64_t *bcols);

/* Pivot log of the last lp_solve / lp_run: (r, c) pairs, oldest first.  The
 * front-end replays it to maintain Simplex._bfs and the variable marks
 * (simplex.py:192-197).  *count = pivots available (may exceed cap). */
int lp_pivot_log(lp_handle *h, int64_t *rc, int64_t cap, int64_t *count);

/* Objective value getZ() = -T[0][0] (tableau.py:82-84, simplex.py:175-179). */
int lp_objective(lp_handle *h, double *z);

/* Pivots deferred into one sweep of the tableau (1..64; 0 = auto, the
 * default: the deepest of 64 / 48 / 32 whose persistent selection still fits
 * one XCD, else 64; lp_get_block reports the value in use).  Each
 * pivot's selection and pivot row use current values computed on the fly; the
 * rank-1 eliminations of `pivots_per_sweep` pivots are applied to the stored
 * tableau in one pass (the same float64 operations in the same order, so the
 * results are identical for every setting).  1 = immediate elimination. */
int lp_set_block(lp_handle *h, int pivots_per_sweep);
int lp_get_block(const lp_handle *h, int *pivots_per_sweep);

/* Device-time accounting of the elimination sweep kernel (for the roofline):
 * enable = 0 off, 1 every launch, k > 1 every k-th launch of each kernel
 * (sampled: fewer events inside a timed loop).  A timed launch records HIP
 * events on the stream it runs on, as part of the launch itself.
 * lp_update_time returns the summed milliseconds and timed launches since the
 * last reset. */
int lp_profile(lp_handle *h, int enable);
int lp_update_time(lp_handle *h, double *ms, int64_t *launches);
/* The same for the pivot-selection launches (one per group of
 * pivots_per_sweep pivots on the single-device path). */
int lp_select_time(lp_handle *h, double *ms, int64_t *launches);

/* Which pivot path the last lp_solve / lp_run of this handle took (extension;
 * the reference is one process on one CPU):
 *   LP_PATH_KERNELS     single device, per-pivot selection kernels
 *   LP_PATH_PERSISTENT  single device, one persistent selection launch per group
 *   LP_PATH_PEER        row-sharded, persistent selection per rank with the
 *                       device-side peer exchange between ranks
 *   LP_PATH_COLLECTIVE  row-sharded, per-pivot kernels + one collective
 *                       exchange per pivot (RCCL, or the host's all-gather)
 * A persistent group whose exchange times out (never expected: the launch is
 * sized from the kernel's occupancy) is redone on the per-pivot kernels and
 * counted in *fallbacks. */
#define LP_PATH_KERNELS 0
#define LP_PATH_PERSISTENT 1
#define LP_PATH_PEER 2
#define LP_PATH_COLLECTIVE 3
int lp_exchange_path(const lp_handle *h, int *path, int *fallbacks);

/* Row-sharded persistent selection (LP_PATH_PEER): the cross-rank hop as
 * this rank's block 0 saw it -- from sending its leaving-row summary (and
 * speculative pivot row) to holding the winner's pivot row -- summed over
 * the handle's pivots: *ticks of the 100 MHz device real-time clock over
 * *pivots pivots (both cumulative since lp_create; read after a call). */
int lp_xwait(const lp_handle *h, int64_t *ticks, int64_t *pivots);

/* Human-readable description of the last failure on this handle (or of the
 * last failed lp_create* when h is NULL). */
const char *lp_last_error(const lp_handle *h);

/* ---- Batched solve: many small LPs of one shape, one workgroup per LP with
 * the LP's whole tableau in LDS (csrc/batch.hip).  Replaces a host loop of
 * Simplex(t).solve() (simplex.py:110-148) over tableaux that each fit one
 * CU's LDS.  One batch lives on one device and holds one shape (a ragged
 * batch, lp_ragged_create further down, holds LPs of many).  lp_batch_solve
 * and lp_batch_run start from the tableau as uploaded (a basic feasible one);
 * lp_twophase_solve, below, runs phase 1 first, on the device as well.
 *
 * What the two paths promise.  Every LP of a batch gets exactly the float64
 * operations of oracle/lp_f64.c on EVERY input, non-finite cells included: a
 * NaN or infinite b, a or c, a negative b, a zero pivot and a ratio that
 * overflows are handled as lpf_solve / lpf_run handle them, pivot for pivot
 * (and, under LP_RULE_MAX_INCREASE, as lpf_find_max_increase + lpf_pivot do).
 * The single-LP engine (lp_create, lp_solve / lp_run) promises the same on
 * FINITE tableaux whose eligible ratios b_i / a_ic stay finite.  Its selection
 * summaries use a ratio of +inf as "no candidate" and clamp the tie band
 * g + tie |g| to DBL_MAX, so it parts from the oracle, and from the batch
 * path, on two inputs:
 *   - an eligible row (a > tol.pivot) whose ratio overflows to +inf is not a
 *     candidate: where every eligible ratio overflows lp_solve answers
 *     LP_UNBOUNDED, while the oracle and the batch pivot on the first such row;
 *   - a finite g so near DBL_MAX that the oracle's band g + tie |g| is +inf
 *     takes such a row in the oracle and the batch, never in the engine.
 * The engine is left as it is: a pivot on an overflowed ratio fills the
 * tableau with inf and NaN, so neither answer is of use to a caller, and a
 * separate has-candidate bit would lengthen every summary on the critical
 * path.  Within the shared domain a batch result is bit-identical to a
 * single-LP lp_solve / lp_run of each LP
 * (tests/test_gpu_engine_contract.py). */
typedef struct lp_batch lp_batch;

/* `count` x Tableau(m, n) (tableau.py:36-52) on one GPU, zeroed; log_cap =
 * (r, c) pairs kept per LP (0: no log).  LP_BAD_ARG, without touching a
 * device, for count/m/n <= 0, log_cap < 0, or a shape whose LDS need --
 * ((m+1) * pitch + pitch + (m+1) + 16) * 8 bytes, pitch = (n+1) | 1 -- exceeds
 * a CU's 160 KiB ("too large for the batch path": use lp_create); also for a
 * shape the device itself will not grant a workgroup. */
int lp_batch_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, lp_batch **out);
int lp_batch_destroy(lp_batch *b);

/* lp_set_tol for every LP of the batch (the lp_tol of lpf_solve / lpf_run). */
int lp_batch_set_tol(lp_batch *b, const lp_tol *tol);

/* Most pivots one kernel launch runs per LP (>= 1; default 4096).  A solve
 * relaunches until every LP is finished; the results do not depend on it. */
int lp_batch_set_chunk(lp_batch *b, int64_t pivots_per_launch);

/* Whole tableaux of LPs [first, first+count): count x (m+1) x ldh doubles,
 * engine layout per LP, ldh >= n+1.  Replace setZ/setC/setB/setA
 * (tableau.py:128-158) and getZ/getC/getB/getA (tableau.py:82-108) for a
 * window of the batch.  An upload resets those LPs' state (counters, log);
 * every other LP is untouched. */
int lp_batch_upload(lp_batch *b, int64_t first, int64_t count, const double *src, int64_t ldh);
int lp_batch_download(lp_batch *b, int64_t first, int64_t count, double *dst, int64_t ldh);

/* Simplex._bfs (simplex.py:192-197) kept on the device: basis is count x m
 * basic columns; every pivot (r, c) of LP i sets basis[i][r] = c.  NULL
 * detaches it.  lp_batch_get_basis copies the current array back. */
int lp_batch_set_basis(lp_batch *b, const int32_t *basis /* count x m, or NULL to detach */);
int lp_batch_get_basis(lp_batch *b, int32_t *basis);

/* Simplex.solve (simplex.py:110-148) per LP, as lp_solve does for one handle
 * and lpf_solve in the oracle: a new solve of every LP from its current
 * tableau.  max_pivots < 0: no cap.  Returns 0 when the call ran -- status[i]
 * is LP i's lp_status (LP_OPTIMAL, LP_UNBOUNDED, LP_CAP_REACHED,
 * LP_OBJ_INCREASED), npiv[i] / nstd[i] its pivots and the standard-rule ones
 * (any of the three may be NULL) -- else a negative lp_status. */
int lp_batch_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int64_t *npiv, int64_t *nstd);

/* k pivots of one rule per LP with no stall logic: findPivotStandard /
 * findPivotMinIndex (simplex.py:218-284) with do_pivot, k times, as lp_run and
 * lpf_run.  status[i] is LP_PIVOTED after k pivots, else LP_OPTIMAL or
 * LP_UNBOUNDED; done[i] = pivots performed.
 *
 * rule = LP_RULE_MAX_INCREASE: findPivotMaxIncrease(do_pivot=True)
 * (simplex.py:286-328), k times, exactly lpf_find_max_increase + lpf_pivot of
 * oracle/lp_f64.c.  One step, in tableau indices (row 0 costs, column 0 b):
 *   - a column j takes part iff T[0][j] < -tol.cost; its g_j is lpf_min_ratio:
 *     from +inf, over the rows with a = T[i][j] > tol.pivot,
 *     q = (|b_i| <= tol.zero ? 0 : b_i) / a, taken iff q < g_j (a NaN or +inf
 *     ratio never is -- not the "first eligible row seeds the minimum" of the
 *     ratio test below);
 *   - any such column with no finite g_j ends the LP LP_UNBOUNDED, whatever the
 *     other columns hold; no such column at all ends it LP_OPTIMAL;
 *   - inc_j = -T[0][j] * g_j (-inf where j does not take part), M their maximum
 *     under inc_j > M from -inf (a NaN is never taken), and the entering column
 *     is the first j with inc_j >= M - tol.ratio_tie * |M|;
 *   - no such j (only with non-finite increases: M = +inf makes the band NaN;
 *     lpf_find_max_increase then returns LP_PIVOTED with c = -1) ends the LP
 *     with status[i] = LP_BAD_PIVOT, no pivot applied;
 *   - the leaving row is the ratio test of the other two rules on that column
 *     (LP_UNBOUNDED where it finds none), then the same pivot, basis and log.
 * With a large k this is a solve to optimality under the max-increase rule
 * (there is no stall logic).  It runs on uniform and ragged batches under
 * every placement; a batch in which some LP has a team above 1
 * (lp_teamed_create*) refuses it with LP_BAD_ARG before any launch -- every
 * workgroup of a team would scan the whole tableau -- and keeps running rules
 * 0 and 1.  lp_batch_solve and the two-phase calls never use it: Simplex.solve
 * is the standard rule, then min-index.
 *
 * rule = LP_RULE_DUAL: k dual simplex pivots per LP, the warm start after
 * lp_resolve_set_rhs (the reference has no dual rule; the pivot is lpf_pivot).
 * The tableau must be dual feasible -- every cost >= -tol.cost -- and may hold
 * negative b.  In tableau indices (row 0 costs, column 0 b):
 *   - at the start of a call only: any T[0][j] < -tol.cost, j = 1..n, ends the
 *     LP with status[i] = LP_BAD_ARG, no pivot applied, whatever k is;
 *   - then, per step, done[i] >= k ends it LP_PIVOTED before any selection;
 *   - leaving row: row i takes part iff b_i = T[i][0] < -tol.zero; g is the
 *     exact minimum of those b_i (from +inf under b_i < g); no such row ends the
 *     LP LP_OPTIMAL; R is the first row that takes part with
 *     b_i <= g + tol.cost_tie * |g|; none (only b = -inf, whose band is NaN)
 *     ends it LP_BAD_PIVOT;
 *   - entering column: column j takes part iff a = T[R][j] < -tol.pivot; its
 *     ratio is q_j = (|c_j| <= tol.cost ? 0.0 : c_j) / (-a), an IEEE division;
 *     g is their minimum from +inf under q < g, so a NaN is never taken; no
 *     such column ends the LP LP_INFEASIBLE (row R proves it: b_R < 0 and no
 *     negative entry); C is the first column that takes part with
 *     q_j <= g + tol.ratio_tie * |g|; none (only NaN ratios) ends it
 *     LP_BAD_PIVOT, no pivot applied;
 *   - lpf_pivot on (R, C), basis[R-1] = C-1 and the log entry, as the other
 *     rules.
 * Both argmins are exact minimum first, then the first index inside the band.
 * There is no anti-cycling logic: k is the guard.  Runs on uniform and ragged
 * batches under every placement; a batch in which some LP has a team above 1
 * refuses it with LP_BAD_ARG before any launch.  lp_batch_solve and the
 * two-phase calls never use it. */
int lp_batch_run(lp_batch *b, int rule, int64_t k, int32_t *status, int64_t *done);

/* getZ() = -T[0][0] of every LP (tableau.py:82-84, as lp_objective). */
int lp_batch_objective(lp_batch *b, double *z /* count */);

/* Pivot log of LP `index` from the last lp_batch_solve / lp_batch_run, as
 * lp_pivot_log (the log of lpf_solve / lpf_run): up to min(cap, log_cap)
 * (r, c) pairs, oldest first; *count = all its pivots (may exceed both). */
int lp_batch_log(lp_batch *b, int64_t index, int64_t *rc, int64_t cap, int64_t *count);

/* As lp_last_error: the last failure on this batch (NULL: the last failed
 * lp_batch_create). */
const char *lp_batch_last_error(const lp_batch *b);

/* ---- Two-phase solve of a batch: Simplex(t) followed by solve()
 * (Simplex._find_bfs simplex.py:36-108, then Simplex.solve simplex.py:110-148)
 * for every LP of an lp_batch, in the same one-workgroup-per-LP kernel family
 * (csrc/batch.hip).  LPs may have rows with b_i < 0 and rows
 * without a unit column.  Per LP the result is oracle/phase1.py's solve_lp bit
 * for bit: rows with b_i < 0 are negated, isCanonical's basic columns are
 * scanned (tableau.py:466-496), rows without one get artificial columns
 * n, n+1, ..., the artificial problem is solved (lpf_solve on m x (n+k), stall
 * switch at m+n+k), basic artificials are pivoted out or their rows dropped,
 * the objective is restored (product rounded before the add, as numpy does),
 * and phase 2 is lpf_solve on the m' x n tableau.  The check of
 * simplex.py:105-106 (the restored tableau is canonical) is not made: phase 2
 * runs on the restored tableau as it is. */
#define LP_STAGE_PHASE2     0   /* simplex.py:110-148 */
#define LP_STAGE_ARTIFICIAL 1   /* simplex.py:49-67   */
#define LP_STAGE_DRIVE_OUT  2   /* simplex.py:68-84   */

/* LDS one workgroup needs for an m x n LP with up to m artificial columns:
 * ((m+1) * pitch + pitch + (m+1) + 16 + (m+1)/2) * 8 bytes with
 * pitch = (n+1+m) | 1 -- lp_batch_create's formula at the widened pitch plus
 * the basis (m int32).  One wave per LP while (m+1) * (n+1+m) <= 2048, four
 * above.  No device is touched.  LP_BAD_ARG for m or n <= 0. */
int64_t lp_twophase_lds_bytes(int64_t m, int64_t n);

/* Replaces the host loop of Simplex(t) + solve() (simplex.py:36-148) over the
 * batch.  max_pivots caps each of the two solves separately (< 0: no cap); the
 * at most m drive-out pivots are not capped.  Returns 0 when the call ran,
 * else a negative lp_status; every output pointer may be NULL.  Per LP:
 *   stage[i]  LP_STAGE_* where the LP ended;
 *   status[i] phase 2: as lp_batch_solve.  Artificial solve: LP_INFEASIBLE
 *             (|T[0][0]| > tol.zero, simplex.py:64-67), LP_CAP_REACHED, or
 *             LP_UNBOUNDED / LP_OBJ_INCREASED (simplex.py:63, "unbounded
 *             artificial problem").  Drive-out: LP_PHASE1_FAILED (a basic
 *             artificial row with |b_i| > tol.zero, simplex.py:73);
 *   rows[i]   m' = m minus the dropped (linearly dependent) rows;
 *   ninit[i]  phase-1 pivots (artificial solve, then drive-out);
 *   npiv[i], nstd[i]  those of phase 2.
 * An LP that reached phase 2 leaves its final (m'+1) x (n+1) tableau in its
 * first m'+1 rows, the rest +0.0; any other LP keeps its uploaded tableau.
 * The call derives the basis itself (replacing one attached with
 * lp_batch_set_basis): lp_batch_get_basis then gives count x m, entries past
 * rows[i] = -1.  lp_batch_log gives the phase-1 pivots followed by the
 * phase-2 ones (*count = ninit + npiv; artificial columns are n, n+1, ...).
 * LP_BAD_ARG ("too large", nothing launched, batch unchanged) when
 * lp_twophase_lds_bytes(m, n) exceeds 160 KiB or what the device grants. */
int lp_twophase_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int32_t *stage,
                      int64_t *rows, int64_t *ninit, int64_t *npiv, int64_t *nstd);

/* ---- Ragged batches: LPs of different shapes in one lp_batch (csrc/batch.hip,
 * csrc/batch_plan.h).  Every LP gets exactly the float64
 * operations of the oracle for its OWN shape -- the stall switch at its own
 * m + n, its artificial columns numbered from its own n, its own odd LDS pitch
 * -- which padding to a common shape does not give.  The LPs are sorted into
 * launch bins by wave count and by how many of them a CU holds, so a small LP
 * is never launched with a large LP's LDS allocation; each solve launches the
 * bins one after the other on the batch's stream.
 *
 * The handle is an lp_batch.  These calls work on it unchanged:
 * lp_batch_set_tol, lp_batch_set_chunk, lp_batch_solve, lp_batch_run,
 * lp_batch_objective, lp_batch_log, lp_batch_last_error, lp_batch_destroy and
 * lp_twophase_solve.  The four whose buffer layout assumes one shape --
 * lp_batch_upload, lp_batch_download, lp_batch_set_basis, lp_batch_get_basis
 * -- return LP_BAD_ARG on a ragged batch and name the call below to use
 * instead.  The calls below take a batch of lp_batch_create as well (its
 * packed layout is ldh = n + 1).
 *
 * lp_ragged_create: `count` LPs, LP i a Tableau(m[i], n[i]), zeroed.
 * LP_BAD_ARG, without touching a device, for count <= 0, a NULL array,
 * log_cap < 0, any m[i] or n[i] <= 0 (the message names i), and for any LP
 * whose LDS need by lp_batch_create's formula exceeds 160 KiB ("too large",
 * with the index of the first such LP). */
int lp_ragged_create(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device,
                     lp_batch **out);
int lp_ragged_shape(const lp_batch *b, int64_t index, int64_t *m, int64_t *n);

/* Whole tableaux of LPs [first, first+count), packed: LP after LP, each
 * (m_i+1) x (n_i+1) row-major, no padding; src / dst point at the first LP of
 * the window.  An upload resets those LPs' state; every other LP is untouched.
 * After lp_twophase_solve an LP that reached phase 2 holds its final
 * (m'+1) x (n_i+1) rows first and +0.0 after, inside its own packed slot. */
int lp_ragged_upload(lp_batch *b, int64_t first, int64_t count, const double *src);
int lp_ragged_download(lp_batch *b, int64_t first, int64_t count, double *dst);

/* lp_batch_set_basis / lp_batch_get_basis, packed: LP i's m_i basic columns
 * after those of the LPs before it, sum of m_i entries (NULL detaches).  After
 * lp_twophase_solve the entries of LP i past rows[i] are -1. */
int lp_ragged_set_basis(lp_batch *b, const int32_t *basis);
int lp_ragged_get_basis(lp_batch *b, int32_t *basis);

/* The launch bins the next plain (twophase = 0) or two-phase (1) call uses, in
 * launch order (largest LDS first): up to cap records of four int64 --
 * {waves per LP, dynamic LDS bytes of the launch, LPs in the bin, LPs of the
 * bin a CU holds}; *count = all bins.  A bin's LDS is the largest need among
 * its LPs; LP i is in the bin keyed (waves_i, min(slot cap of that wave
 * count, floor(160 KiB / need_i))).  LP_BAD_ARG ("too large", with the LP's
 * index) when twophase = 1 and an LP's lp_twophase_lds_bytes exceeds 160 KiB;
 * lp_twophase_solve refuses such a batch in the same way, before any launch,
 * and the batch stays usable for lp_batch_solve. */
int lp_ragged_plan(lp_batch *b, int twophase, int64_t *bins, int64_t cap, int64_t *count);

/* ---- Placed batches: LPs too large for a CU's LDS (csrc/batch.hip
 * k_batch_dev, csrc/batch_plan.h).  A placed batch may keep an
 * LP's tableau in device memory for the whole launch: still one workgroup per
 * LP, no communication between workgroups, the same chunked launches and the
 * same float64 operations as oracle/lp_f64.c; only the pivot row, the
 * multipliers and the reduction scratch are in LDS.
 *
 * lp_placed_create / lp_placed_create_ragged are lp_batch_create /
 * lp_ragged_create with a placement request; LP_PLACE_LDS is the old call,
 * refusals and messages included.  LP_BAD_ARG, without touching a device, for
 * an unknown `place`, for everything the old calls refuse for other reasons,
 * and for a device-placed LP whose side buffers, lp_placed_lds_bytes(m,
 * n) = ((n+1) + (m+1) + 16) * 8, exceed 160 KiB ("too large", with the LP's
 * index on a ragged batch): m + n of about 20,000.
 *
 * The stored layout is the same: every data, basis, objective, log, tolerance
 * and chunk call works on a placed batch unchanged.  Placement governs
 * lp_batch_solve and lp_batch_run only.  lp_twophase_solve keeps its own LDS
 * test: it runs on any batch whose LPs fit lp_twophase_lds_bytes, whatever the
 * placement, and refuses "too large" otherwise, before any launch.
 *
 * A launch of device-placed LPs runs at most min(chunk, W / ((m+1)(n+1)))
 * pivots per LP, at least one (W: DESIGN.md 4j), so that a large LP does not
 * hold a CU for long; results do not depend on it.
 *
 * lp_ragged_plan(b, 0, ...) lists the device-placed LPs as one bin, first (it
 * is launched first): {waves per LP, the largest side-buffer need among its
 * LPs, its LP count, the LPs of it a CU holds}.  The LDS-placed LPs are binned
 * as in lp_ragged_create's batch. */
#define LP_PLACE_LDS    0   /* as lp_batch_create / lp_ragged_create: refuse an LP above a CU's LDS */
#define LP_PLACE_AUTO   1   /* LDS where the LP fits (lp_batch_create's formula), device memory where not */
#define LP_PLACE_DEVICE 2   /* device memory for every LP (tests, A/B) */
int lp_placed_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, int place,
                           lp_batch **out);
int lp_placed_create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device,
                            int place, lp_batch **out);
/* LP_PLACE_LDS or LP_PLACE_DEVICE: what LP `index` got */
int lp_placed_placement(const lp_batch *b, int64_t index, int *place);
/* LDS bytes of one device-placed m x n LP (LP_BAD_ARG for m or n <= 0) */
int64_t lp_placed_lds_bytes(int64_t m, int64_t n);

/* ---- Phased batches: the two-phase solve of LPs whose widened tableau does
 * not fit a CU's LDS (csrc/batch.hip k_twophase_dev, csrc/batch_plan.h,
 * DESIGN.md 4k).  lp_twophase_solve needs (m+1) x (n+1+m) float64 in LDS; an
 * LP above that runs the same stages with its working tableau in device
 * memory for the whole call, contiguous at its live width (n+1+k, then n+1),
 * one workgroup per LP, and gives the same bits: oracle/phase1.py's solve_lp.
 *
 * lp_phased_solve replaces the host loop of Simplex(t) + solve()
 * (simplex.py:36-148) over the batch, as lp_twophase_solve does, and takes its
 * eight arguments with the same meaning.  Each LP is placed under the batch's
 * creation-time request (lp_placed_create): LP_PLACE_LDS is lp_twophase_solve
 * itself, refusal included; LP_PLACE_AUTO keeps an LP in LDS exactly when
 * lp_twophase_lds_bytes(m, n) <= 160 KiB and in device memory otherwise;
 * LP_PLACE_DEVICE keeps every LP in device memory.  An LP can therefore be
 * LDS-placed for lp_batch_solve and device-placed here.  LP_BAD_ARG ("too
 * large", with the LP's index, nothing launched, the batch still usable) when
 * a device-placed LP's lp_phased_lds_bytes exceeds 160 KiB.
 *
 * A launch of device-placed LPs runs at most min(chunk, W / ((m+1)(n+1+m)))
 * pivots per LP, at least one, drive-out pivots included (W: DESIGN.md 4j);
 * results do not depend on it. */
int lp_phased_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int32_t *stage,
                    int64_t *rows, int64_t *ninit, int64_t *npiv, int64_t *nstd);
/* LDS bytes of one device-placed two-phase m x n LP: the pivot row at the
 * widest live width, the multipliers, the reduction scratch and the basis,
 * ((n+1+m) + (m+1) + 16 + (m+1)/2) * 8 (LP_BAD_ARG for m or n <= 0) */
int64_t lp_phased_lds_bytes(int64_t m, int64_t n);
/* LP_PLACE_LDS or LP_PLACE_DEVICE: where lp_phased_solve runs LP `index`
 * (LP_BAD_ARG where neither placement the batch allows takes it) */
int lp_phased_placement(const lp_batch *b, int64_t index, int *place);
/* The launch bins of lp_phased_solve in lp_ragged_plan's format; the
 * device-placed LPs are one bin, first: {waves per LP, the largest
 * lp_phased_lds_bytes among its LPs, its LP count, the LPs of it a CU holds} */
int lp_phased_plan(lp_batch *b, int64_t *bins, int64_t cap, int64_t *count);

/* ---- Teamed batches: several workgroups per LP when the batch is small
 * (csrc/batch.hip k_batch_team, csrc/batch_plan.h).  A
 * device-placed LP is bound by what one workgroup moves through memory, however
 * few LPs the batch holds.  A teamed LP is worked on by G workgroups: one
 * launch applies one pivot; every workgroup of the team selects the pivot
 * itself on the LP's current tableau and writes its own contiguous range of
 * the updated tableau into the LP's second buffer.  Nothing waits on another
 * workgroup; the launches on the batch's stream are the only ordering.  The
 * results are the bits of lp_placed_create's batch: oracle/lp_f64.c.
 *
 * lp_teamed_create / lp_teamed_create_ragged are lp_placed_create /
 * lp_placed_create_ragged with a team request: 1 is the placed batch itself; 0
 * (auto) gives a device-placed LP of E = (m+1)(n+1) elements, D device-placed
 * LPs in the batch, clamp(min(slots / D, E / LPK_TEAM_MIN_ELEMS), 1,
 * LPK_TEAM_MAX) workgroups, slots being the chip's resident workgroups of the
 * kernel, and 1 where D > E / LPK_TEAM_LP_ELEMS: a team where it was measured
 * to pay, 1 where not; G > 1 asks for G.  The ragged call takes
 * one request per LP (NULL: 1 for all).  A teamed LP is always device-placed:
 * under LP_PLACE_AUTO a request G > 1 places the LP in device memory, and an LP
 * that auto placement keeps in LDS has team 1.  LP_BAD_ARG, without touching
 * a device: a negative request; G > 1 with LP_PLACE_LDS; G above LPK_TEAM_MAX
 * or above (m+1)(n+1) / 2; and everything lp_placed_create refuses.  The second
 * tableau buffer exists only where some LP got a team above 1.
 *
 * Teams govern lp_batch_solve and lp_batch_run only; every data, basis, log,
 * objective, tolerance and chunk call works unchanged, and lp_twophase_solve
 * and lp_phased_solve ignore teams.  lp_ragged_plan(b, 0, ...) lists the LPs of
 * team 1 only. */
int lp_teamed_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, int place, int team,
                     lp_batch **out);
int lp_teamed_create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device,
                            int place, const int32_t *team, lp_batch **out);
/* the workgroups LP `index` got (1: not teamed) */
int lp_teamed_size(const lp_batch *b, int64_t index, int *team);
/* The workgroup table of a teamed launch, LPs ascending, ranks in order: rows
 * of five, {LP, rank, team, first element, one past the last element} of the
 * LP's (m+1)(n+1); *count = the workgroups of a launch (0: no LP is teamed) */
int lp_teamed_plan(lp_batch *b, int64_t *rows, int64_t cap, int64_t *count);
/* launches enqueued per read-back of the records, >= 1 (the teamed form of
 * lp_batch_set_chunk: a launch is one pivot); results do not depend on it */
int lp_teamed_set_window(lp_batch *b, int64_t launches_per_readback);

/* ---- Batch solutions on the device: the starting basis and x without the
 * tableau (csrc/batch.hip k_canon_*, k_solution; csrc/batch_plan.h; DESIGN.md
 * 4m).  Both calls work on any lp_batch -- uniform or ragged, LDS- or
 * device-placed, teamed or not -- and read only the packed tableaux as stored
 * and the basis array; nothing waits on another workgroup, the launches on
 * the batch's stream are the only ordering.  A family of their own, lp_solution_*,
 * as lp_ragged_* and the later ones are: the lp_batch_* set is closed. */

/* Tableau.isCanonical's basic column per row (tableau.py:466-496), on the
 * device, for LPs [first, first+count) from their tableaux as stored now
 * (after an upload, or after a solve).  Column j in 0..n-1 is basic for row i
 * when c_j == 0.0, a_ij == 1.0 and every other entry of the column == 0.0 (a
 * NaN is nonzero); the lowest such column wins a row, a row without one gets
 * -1.  The result is written into the batch's device basis array, packed as
 * lp_ragged_set_basis takes it (count x m on a uniform batch), and the basis
 * becomes attached as after lp_batch_set_basis; if none was attached before,
 * the entries of the LPs outside the window are -1.  flags[i] of window LP i:
 * bit 0, some b_r < 0.0 (an exact compare: -0.0 and NaN do not set it); bit 1,
 * some row got -1.  *first_bad = the batch index of the first LP of the window
 * with a nonzero flag, or -1.  Returns LP_PIVOTED whether or not an LP is bad:
 * the caller decides (lp_batch_solve does not look).  LP_BAD_ARG, nothing
 * launched: NULL batch, window out of bounds.  count == 0 is a no-op. */
int lp_solution_canonical(lp_batch *b, int64_t first, int64_t count,
                       int32_t *flags /* count, may be NULL */, int64_t *first_bad /* may be NULL */);

/* Simplex.getBFS (simplex.py:166-173) and getObjValue (:175-179) for LPs
 * [first, first+count), gathered on the device from the stored tableaux and
 * the attached basis (LP_BAD_ARG without one, as lp_batch_get_basis).  x is
 * packed: LP i's n_i doubles after those of the window's LPs before it (count
 * x n on a uniform batch); every entry +0.0, then for r = 0..m_i-1 in row
 * order x[basis[r]] = T[1+r][0] -- a later row overwrites an earlier one with
 * the same column, an entry outside [0, n_i) is skipped (the -1 entries past
 * rows[i] after a two-phase call).  z[i] = -T[0][0], the bits of
 * lp_batch_objective.  Defined for every LP whatever its status; writes
 * nothing but a staging buffer the batch owns. */
int lp_solution_gather(lp_batch *b, int64_t first, int64_t count,
                      double *x /* packed, may be NULL */, double *z /* count, may be NULL */);

/* ---- Problem-form batches: tableaux built on the device from c, A, b and one
 * sense per row, and the duals read back without the tableau (csrc/batch.hip
 * k_assemble, k_duals; csrc/batch_plan.h).  The LP is
 *     min c.x   subject to   A x {<=, >=, ==} b,   x >= 0
 * with m rows and ns structural variables.  Its problem block P is the
 * row-major (m+1) x (ns+1) float64 array of the first ns + 1 tableau columns:
 * P[0][0] the stored _z cell, P[0][1+j] = c_j, P[1+i][0] = b_i,
 * P[1+i][1+j] = a_ij.  The assembled tableau is (m+1) x (n+1), n = ns + k, k
 * the rows that are not equalities: columns 0..ns are P's 64-bit patterns; the
 * t-th row r that is not an equality (from 0, in row order) owns variable column
 * ns + t, where T[1+r][1+ns+t] is +1.0 for <= and -1.0 for >=; every other
 * cell is +0.0.  The calls work on any lp_batch -- uniform or ragged, LDS- or
 * device-placed, teamed or not.  A family of its own, as lp_solution_* is. */
#define LP_SENSE_LE 0
#define LP_SENSE_GE 1
#define LP_SENSE_EQ 2

/* n = ns + k for m senses: the host's slack layout around setA
 * (tableau.py:150-158) as a count, so that lp_*_create can be sized.  No
 * device is touched.  LP_BAD_ARG: NULL, m or ns <= 0, a sense outside 0..2. */
int64_t lp_problem_columns(const int8_t *sense, int64_t m, int64_t ns);

/* The senses of the batch's LPs, in place of the slack and surplus columns a
 * caller of setA lays out by hand (tableau.py:150-158): m entries shared by
 * every LP of a uniform batch; packed on a ragged one, LP i's m_i entries
 * after those of the LPs before it, as lp_ragged_set_basis.  NULL detaches
 * them; a second call replaces them.  LP_BAD_ARG with nothing changed -- the
 * message names the LP and the row -- for a sense outside 0..2, and for an LP
 * with k_i >= n_i, which would leave no structural variable. */
int lp_problem_set_senses(lp_batch *b, const int8_t *sense);

/* ns_i = n_i - k_i of LP `index`: the reference's count of structural
 * variables, Tableau.getTableauSize()[1] (tableau.py:78-80) less the slacks.
 * LP_BAD_ARG without senses. */
int lp_problem_vars(const lp_batch *b, int64_t index, int64_t *ns);

/* Problem blocks of LPs [first, first+count), packed LP after LP without
 * padding.  Replaces setZ/setC/setB/setA (tableau.py:128-158) plus the host's
 * slack layout: one copy into a staging buffer the batch owns, one launch of
 * k_assemble that writes the window's tableaux, a stream synchronise.  The
 * state afterwards is that of lp_batch_upload / lp_ragged_upload of the
 * assembled tableaux: those LPs' records and logs reset, every other LP
 * untouched bit for bit.  LP_BAD_ARG, nothing copied or launched: NULL batch,
 * no senses attached, window out of bounds, src NULL with count > 0.
 * count == 0 is a no-op. */
int lp_problem_upload(lp_batch *b, int64_t first, int64_t count, const double *src);

/* The dual values of LPs [first, first+count) from row 0 of their stored
 * tableaux, where the reference reads them with getCj (tableau.py:86-92)
 * under the slack columns: y packed, m_i per LP (count x m on a uniform
 * batch), indexed by the rows of the uploaded problem.  A row r that owns
 * column j gives y[r] = -T[0][1+j] for <= (a flip of the sign bit) and
 * T[0][1+j] for >=; an equality row gives the quiet NaN 0x7ff8000000000000
 * (its artificial column is gone after phase 1).  The column does not move
 * when phase 1 negates or drops rows, so this holds after lp_twophase_solve /
 * lp_phased_solve unchanged; defined for every LP whatever its status.  For
 * the minimisation solved: y <= 0 on <= rows, y >= 0 on >= rows, b.y = z at an
 * optimum.  Writes nothing but a staging buffer the batch owns.  LP_BAD_ARG
 * without senses. */
int lp_problem_duals(lp_batch *b, int64_t first, int64_t count, double *y);

/* ---- Warm re-solves: new right-hand sides on the stored tableaux, then
 * lp_batch_run with LP_RULE_DUAL from the basis they hold (csrc/batch.hip
 * k_rhs, bdual; csrc/batch_plan.h).  After any sequence of pivots
 * -- phase 1's row negations included -- a stored tableau is M . [the assembled
 * tableau] for an invertible M, and the column that row k's slack or surplus
 * variable owns holds M's column of that row up to the sign s_k = +1 (<=) or
 * -1 (>=).  So the column 0 that the same pivots would have left had the LP
 * been uploaded with other right-hand sides is M . rhs.  Row 0 does not change:
 * an optimal tableau stays dual feasible and may turn primal infeasible, the
 * dual simplex's starting point.
 *
 * rhs is packed, m_i + 1 doubles per LP of [first, first+count): the new
 * column 0 of the LP's problem block, rhs[0] the stored _z cell, rhs[1+k] =
 * b_k.  One copy into a staging buffer the batch owns, one launch of k_rhs, a
 * stream synchronise.  Per tableau row i = 0..m_i, with slack[k] = +-(1 + j_k)
 * the table of lp_problem_set_senses:
 *     acc = (i == 0 ? rhs[0] : +0.0)
 *     for k = 0 .. m_i - 1:  acc = acc + (s_k * T[i][1+j_k]) * rhs[1+k]
 *     T[i][0] = acc
 * every product and every sum rounded on its own (no fma), the product with
 * s_k a flip of the sign bit.  Nothing else changes: every other cell, the
 * basis, the records and the logs stay, and so do the LPs outside the window.
 * Valid whatever the LP's status.  LP_BAD_ARG, nothing copied or launched, the
 * message naming the LP and the row: no senses attached, an LP of the window
 * with an == row (it owns no column, as for its dual), an LP whose last
 * two-phase call left fewer than m_i live rows, window out of bounds, rhs NULL
 * with count > 0.  count == 0 is a no-op.  A family of its own: the lp_problem_*
 * names are a closed set. */
int lp_resolve_set_rhs(lp_batch *b, int64_t first, int64_t count, const double *rhs);

/* ---- General-form batches: variable bounds, free variables and maximise,
 * converted to the standard form on the device and undone there (csrc/batch.hip
 * k_general_shift, k_general_assemble, k_general_recover, k_general_duals;
 * csrc/batch_plan.h).  The LP is
 *     min or max  c0 + c.x   subject to   A x {<=, >=, ==} b
 * with m rows, ns variables and one kind per variable (LP_VAR_*): x_j >= 0,
 * x_j >= lb_j (x = lb + x'), lb_j <= x_j <= ub_j (x = lb + x' and a row
 * x' <= ub - lb), x_j <= ub_j (x = ub - x') or free (x = x+ - x-).  With nf
 * FREE and nb BOXED variables and k rows that are not equalities the standard
 * form has m' = m + nb rows, the bound rows after the m rows in variable order,
 * each a <= row, and n' = ns + nf + k + nb columns: the ns variables, the
 * negative parts of the FREE ones in variable order, then the slack columns
 * of lp_problem_set_senses over the m' senses.  The batch is created at
 * (m', n') with the existing create calls.  The general block of an LP is its
 * problem block P, (m+1) x (ns+1) with P[0][0] = -c0, then lb[ns], then ub[ns];
 * a bound its kind does not use is not read.  Cell by cell (a flip is a flip
 * of the sign bit, every product is rounded before its subtraction, s_j = lb_j
 * for LOWER and BOXED, ub_j for UPPER): T[0][1+j] = c_j flipped iff (maximise
 * XOR UPPER), a FREE negative part that cell flipped once more; T[1+i][1+j] =
 * a_ij flipped iff UPPER, a FREE negative part a_ij flipped; T[1+i][0] = b_i
 * less a_ij * s_j for the shifted j ascending; T[0][0] = P[0][0] flipped iff
 * maximise, less cs_j * s_j likewise, cs_j = c_j flipped iff maximise; a bound
 * row holds ub_j - lb_j, +1.0 under variable j and under its slack.  With every
 * kind LP_VAR_PLAIN under min these are lp_problem_upload's tableaux bit for
 * bit.  lb > ub is not refused: the LP ends LP_INFEASIBLE in phase 1.  The
 * calls work on any lp_batch, as lp_problem_*; a family of its own. */
#define LP_VAR_PLAIN 0
#define LP_VAR_LOWER 1
#define LP_VAR_BOXED 2
#define LP_VAR_UPPER 3
#define LP_VAR_FREE 4

/* m' = m + nb and n' = ns + nf + k + nb for m senses and ns kinds, so that
 * lp_*_create can be sized.  No device is touched.  LP_BAD_ARG: NULL, m or
 * ns <= 0, a sense outside 0..2, a kind outside 0..4. */
int64_t lp_general_rows(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns);
int64_t lp_general_columns(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns);

/* The form of the batch's LPs.  A uniform batch takes one m, one ns, m senses,
 * ns kinds and one maximise flag (0 or 1), shared by every LP; a ragged batch
 * count entries of m, ns and maximise, and senses and kinds packed, LP i's m_i
 * and ns_i entries after those of the LPs before it.  m and ns are given
 * because (m', n') alone do not tell where one LP's entries end.  sense NULL
 * detaches the form; a second call replaces it, and what was uploaded under
 * the old one is forgotten.  LP_BAD_ARG with nothing changed -- the message
 * names the LP and the entry -- for a code out of range, and for an LP whose
 * lp_general_rows / lp_general_columns are not the batch's (m_i, n_i). */
int lp_general_set_form(lp_batch *b, const int64_t *m, const int64_t *ns, const int8_t *sense,
                        const int8_t *kind, const int8_t *maximise);

/* m_i and ns_i of LP `index` as the caller states it.  LP_BAD_ARG without a
 * form. */
int lp_general_vars(const lp_batch *b, int64_t index, int64_t *m, int64_t *ns);

/* General blocks of LPs [first, first+count), packed LP after LP without
 * padding: one copy into a staging buffer the batch owns, one launch of
 * k_general_shift (each LP's shifted column 0, one lane per row, the loops
 * above in their stated order), one of k_general_assemble, a stream
 * synchronise.  The state afterwards is that of lp_batch_upload /
 * lp_ragged_upload of the standard-form tableaux: those LPs' records and logs
 * reset, every other LP untouched bit for bit.  The staging buffer holds every
 * LP's block at its own place, so the window's bounds stay on the device for
 * lp_general_solution; windows may arrive in any order, and a second upload
 * replaces its own window only.  LP_BAD_ARG, nothing copied or launched: NULL
 * batch, no form attached, window out of bounds, src NULL with count > 0.
 * count == 0 is a no-op. */
int lp_general_upload(lp_batch *b, int64_t first, int64_t count, const double *src);

/* x and the objective of LPs [first, first+count) in the caller's terms:
 * lp_solution_gather's kernel, then k_general_recover on the same stream.  x
 * is packed, ns_i per LP: the bits of x'_j for PLAIN, lb_j + x'_j for LOWER
 * and BOXED, ub_j - x'_j for UPPER, x'_j - x'_neg(j) for FREE.  z[i] is
 * -T[0][0] under min and the bits of T[0][0] under max.  Needs an attached
 * basis, as lp_solution_gather, and an lp_general_upload under this form.
 * LP_BAD_ARG, nothing launched: NULL batch, no form, window out of bounds. */
int lp_general_solution(lp_batch *b, int64_t first, int64_t count,
                        double *x /* packed, may be NULL */, double *z /* count, may be NULL */);

/* Duals and reduced costs of LPs [first, first+count) for the LP as the caller
 * stated it, from row 0 of the stored tableaux: y packed, m_i per LP, is
 * lp_problem_duals' value of the m original rows flipped iff maximise, an
 * equality row the quiet NaN 0x7ff8000000000000; r packed, ns_i per LP, is
 * T[0][1+j], less the cell under the slack of its bound row for BOXED, flipped
 * iff (maximise XOR UPPER).  At an optimum c - A^T y = r over the rows with a
 * dual; under min r_j >= 0 at a lower bound and <= 0 at an upper one, under
 * max the reverse.  LP_BAD_ARG, nothing launched: NULL batch, no form, window
 * out of bounds. */
int lp_general_duals(lp_batch *b, int64_t first, int64_t count,
                     double *y /* packed, may be NULL */, double *r /* packed, may be NULL */);

/* ---- Warm re-optimisation: new costs, and new bounds and right-hand sides on
 * general-form LPs, on the stored tableaux (csrc/batch.hip k_cost,
 * k_general_restage; csrc/batch_plan.h).  A family of its own:
 * the lp_resolve_* and lp_problem_* names are closed sets.
 *
 * New costs.  A stored tableau is primal feasible for any cost vector if it was
 * for one; only row 0 depends on c, and it is the cost row less c_B times the
 * rows of the basis.  costs is packed, n_i + 1 doubles per LP of [first,
 * first+count): the new row 0 of the tableau as it would be uploaded, costs[0]
 * the stored _z cell (-c0), costs[1+j] the cost of tableau column j, slack and
 * surplus columns included (+0.0 for them).  One copy into a staging buffer the
 * batch owns, one launch of k_cost, a stream synchronise.  Per tableau column
 * j = 0..n_i, with basis[] the attached basis:
 *     acc = costs[j]
 *     for r = 0 .. m_i - 1:
 *         k = basis[r];  if k < 0 or k >= n_i: continue
 *         acc = acc - costs[1+k] * T[1+r][j]
 *     T[0][j] = acc
 * every product and every difference rounded on its own (no fma), rows
 * ascending.  Nothing else changes: rows 1..m, the basis, the records, the logs
 * and the LPs outside the window stay.  A basic column gets what the loop gives:
 * 0.0 on a finite tableau, since lpf_pivot leaves exact unit columns.  Valid
 * whatever the LP's status, on any lp_batch -- tableau- or problem-form, uniform
 * or ragged, LDS- or device-placed, teamed or not (a teamed LP is home in the
 * first buffer between calls).  lp_batch_solve goes on from there.  LP_BAD_ARG,
 * nothing copied or launched, the message naming the LP: no basis attached, an
 * LP whose last two-phase call left fewer than m_i live rows, window out of
 * bounds, costs NULL with count > 0.  count == 0 is a no-op.  Senses are not
 * needed, and == rows are no obstacle. */
int lp_reopt_set_costs(lp_batch *b, int64_t first, int64_t count, const double *costs);

/* New c, b, lb and ub on general-form LPs whose kinds stay: a change of the
 * standard form's right-hand sides (the shifted column and the bound rows'
 * ub - lb) and of its costs.  src is packed, 3 ns_i + m_i + 1 doubles per LP:
 * the border of the LP's general block -- row 0 of P (-c0, then c: ns + 1), b
 * (m), lb (ns), ub (ns).  On the batch's stream: k_general_restage scatters the
 * border into the stored general blocks (A stays), k_general_shift recomputes
 * the window's shifted columns, and k_rhs sets column 0 of the stored tableaux
 * to M . shift over the m' rows, as lp_resolve_set_rhs does with a staged rhs;
 * then a stream synchronise.  lp_batch_run with LP_RULE_DUAL goes on from
 * there.  Row 0 of the tableau is touched in its cell 0 only: if c in src
 * differs from the stored c, the caller must follow with lp_reopt_set_costs
 * (row 0 of the standard form as costs) before any run; the Python layer does
 * that for its callers.  LP_BAD_ARG before anything is copied, the message
 * naming the LP and the variable or row: no form attached, nothing uploaded
 * under it, a bound that does not fit the variable's kind (a NaN; PLAIN needs
 * lb == 0 and ub == +inf, LOWER a finite lb and ub == +inf, BOXED both finite,
 * UPPER lb == -inf and a finite ub, FREE both infinite), an == row among the m
 * rows, an LP whose last two-phase call left fewer than m' live rows, window
 * out of bounds, src NULL with count > 0.  count == 0 is a no-op.  lb > ub on a
 * BOXED variable is not refused: its bound row gets a negative right-hand side
 * and the dual run ends the LP LP_INFEASIBLE. */
int lp_reopt_set_general(lp_batch *b, int64_t first, int64_t count, const double *src);

/* ---- Warm cuts: rows appended to solved LPs, then the dual simplex
 * (csrc/batch.hip k_cut_copy, k_cut_rows, k_cut_basis; csrc/batch_plan.h;
 * DESIGN.md 4s).  A family of its own, as the sets above are closed.
 *
 * A batch has a fixed shape, so the extended LPs go into a second batch: src and
 * dst are two batches on one device with the same LP count, dst made by any of
 * the create calls, under any placement or team, uniform or ragged whatever src
 * is.  For every LP i of [first, first+count), q_i = m'_i - m_i = n'_i - n_i
 * >= 0 rows are added; q_i = 0 copies the LP.  rows is packed LP after LP: q_i
 * stated rows of n_i + 1 doubles, in tableau columns as lp_reopt_set_costs takes
 * costs -- row[0] = beta, row[1+j] the coefficient of tableau column j, slack
 * and surplus columns included (a Gomory cut is stated on them).  sense is
 * packed, q_i entries of LP_SENSE_LE / LP_SENSE_GE per LP.  With T the stored
 * (m+1) x (n+1) tableau of src and basis[] its attached basis, the destination
 * (m+q+1) x (n+q+1) tableau D is
 *     D[i][j]         = the 64 bits of T[i][j]               i <= m, j <= n
 *     D[i][1+n+k]     = +0.0                                 i <= m
 *     D[1+m+k][1+n+k'] = +1.0 if k' == k, else +0.0
 * and for new row k and j = 0..n
 *     acc = row_k[j]
 *     for r = 0 .. m - 1:
 *         c = basis[r];  if c < 0 or c >= n: continue
 *         acc = acc - row_k[1+c] * T[1+r][j]
 *     D[1+m+k][j] = acc, its sign bit flipped iff sense_k is LP_SENSE_GE
 * every product and every difference rounded on its own (no fma), rows
 * ascending: the order is the contract.  dst's basis for the LP is basis[0..m-1]
 * followed by n + k for row k, and it becomes attached; if none was attached
 * before, the entries of the LPs outside the window are -1, as
 * lp_solution_canonical leaves them.  Row 0 is src's, so D is dual feasible
 * where T was, and lp_batch_run(dst, LP_RULE_DUAL, k, ...) goes on from it.  The
 * new columns are where lp_problem_set_senses puts the slacks of m + q senses, so
 * lp_problem_duals, lp_resolve_set_rhs and lp_reopt_set_costs work on dst.
 *
 * For the window's LPs dst's state is that of an upload of D: records, logs and
 * the short-row flag are reset.  Every other LP of dst is untouched bit for bit,
 * and src is not changed at all.  Valid whatever the LPs' status, on tableau-,
 * problem- or general-form sources, with == rows, on teamed sources (a team's LP
 * is home in the first buffer between calls).  The call runs on dst's stream:
 * one copy of rows, one of the window's offsets and senses, into staging dst
 * owns, three launches, one stream synchronise.
 *
 * LP_BAD_ARG, nothing copied or launched and dst unchanged, the message on dst
 * naming the LP (and the row where there is one): a NULL batch; src == dst;
 * different devices or counts; window out of bounds; rows or sense NULL while
 * some q_i > 0; an LP whose m'_i - m_i differs from n'_i - n_i or is negative; a
 * sense outside {LE, GE} (an equality owns no column); no basis attached to
 * src; an LP of src whose last two-phase call left fewer than m_i live rows;
 * senses attached to dst that disagree with the call -- the entry of row
 * m_i + k must be the column 1 + n_i + k with the sign of the given sense, and
 * where src has senses too the first m_i entries must be src's.  count == 0 is
 * a no-op. */
int lp_cut_extend(lp_batch *src, lp_batch *dst, int64_t first, int64_t count, const double *rows,
                  const int8_t *sense);

#ifdef __cplusplus
}
#endif
#endif /* LPGPU_H */
